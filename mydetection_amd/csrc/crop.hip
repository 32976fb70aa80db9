// Object chips: the image of every detection, cut out of uint8 RGB frames or of the planes of the 4:2:0 layouts, turned upright
// and resampled to one fixed size, one launch per batch (include/mydet.h: mydet_crop_boxes_rgb, mydet_crop_boxes_yuv420, where
// the sampling rules are; DESIGN.md has them too).  Built with -ffp-contract=off: the sample coordinates are float32 expressions
// that must not be fused.
//
// grid = (tiles of a chip, M slots, B frames), 256 lanes.  A workgroup owns 256 groups of 4 neighbouring chip pixels of a row
// (the chip's rows cut into groups, groups numbered row by row): 1024 pixels.  They are sampled with neighbouring lanes on
// neighbouring chip pixels (taps that share cache lines) and cross through LDS to the store layout, where a lane stores 16 bytes
// into each float plane, or 12 bytes of packed pixels.  A workgroup of a slot at or beyond the frame's count returns after
// reading the count: such a slot is not written.  Source taps are plain global loads (the taps of a chip overlap and hit L2); a
// tap is tested against the H x W view before it addresses anything, and reads the fill colour outside it.  The 4:2:0 form
// converts every tap with yuv_pixel (yuv_fetch.h): the table, the formula and the 10-bit rule of yuv420.hip.
#include "paint_tile.h"
#include "yuv_fetch.h"

namespace {

constexpr int CR_THREADS = 256;
constexpr float CR_MAX_Q = 536870912.0f;         // 2^29: quantised coordinates beyond +-2^24 pixels are outside every view

struct CropArgs {
    mydet_draw_list l;
    int H, W;
    const unsigned char *src;                    // RGB frames (SRC 0)
    int64_t img, row;
    YuvSrc y;                                    // 4:2:0 planes (SRC 1..4)
    int ch, cw, M, norm;
    float pad;
    uint32_t fill;                               // r | g << 8 | b << 16
    float mean[3], sd[3];
    void *out;
    int64_t slot, frame;                         // elements between the chips of a frame / between frames
    int wide;                                    // 16-byte (float planes) or dword (packed pixels) stores are aligned
};

// SRC: 0 RGB; 1 + 2 * (BPS - 1) + PLANAR for the 4:2:0 fetch.  The pixel at (y, x), which the caller has tested to be inside.
template <int SRC>
__device__ __forceinline__ uint32_t crop_pixel(const CropArgs &p, int b, int y, int x) {
    if constexpr (SRC == 0) {
        const unsigned char *s = p.src + (int64_t)b * p.img + (int64_t)y * p.row + (int64_t)x * 3;
        return px_pack(s[0], s[1], s[2]);
    } else {
        return yuv_pixel<1 + ((SRC - 1) >> 1), ((SRC - 1) & 1) != 0>(p.y, b, y, x);
    }
}

// The pixels (y, x0) and (y, x0 + 1) of frame b; whatever lies outside the view is the fill colour and is not addressed.  An
// RGB pair inside the view is two dword reads, bytes [3*x0, 3*x0 + 4) and [3*x0 + 2, 3*x0 + 6): both end inside the pair.
template <int SRC>
__device__ __forceinline__ void crop_pair(const CropArgs &p, int b, int y, int x0, uint32_t &pa, uint32_t &pb) {
    pa = p.fill;
    pb = p.fill;
    if ((unsigned)y >= (unsigned)p.H) return;
    if constexpr (SRC == 0) {
        if (x0 >= 0 && x0 + 1 < p.W) {
            const unsigned char *s = p.src + (int64_t)b * p.img + (int64_t)y * p.row + (int64_t)x0 * 3;
            uint32_t lo, hi;
            __builtin_memcpy(&lo, s, 4);
            __builtin_memcpy(&hi, s + 2, 4);
            pa = lo & 0xffffffu;
            pb = hi >> 8;
            return;
        }
    }
    if ((unsigned)x0 < (unsigned)p.W) pa = crop_pixel<SRC>(p, b, y, x0);
    if ((unsigned)(x0 + 1) < (unsigned)p.W) pb = crop_pixel<SRC>(p, b, y, x0 + 1);
}

// The 8-bit bilinear value of one sub-sample at (X, Y), three channels into acc
template <int SRC>
__device__ __forceinline__ void crop_sample(const CropArgs &p, int b, float X, float Y, int *acc) {
    const float tx = floorf((X - 0.5f) * 32.0f + 0.5f), ty = floorf((Y - 0.5f) * 32.0f + 0.5f);
    uint32_t p00 = p.fill, p01 = p.fill, p10 = p.fill, p11 = p.fill;
    int fx = 0, fy = 0;
    if (fabsf(tx) <= CR_MAX_Q && fabsf(ty) <= CR_MAX_Q) {                 // false for NaN
        const int qx = (int)tx, qy = (int)ty;
        const int x0 = qx >> 5, y0 = qy >> 5;
        fx = qx & 31; fy = qy & 31;
        if (x0 >= -1 && x0 < p.W && y0 >= -1 && y0 < p.H) {               // else all four taps are outside
            crop_pair<SRC>(p, b, y0, x0, p00, p01);
            crop_pair<SRC>(p, b, y0 + 1, x0, p10, p11);
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int top = px_chan(p00, c) * (32 - fx) + px_chan(p01, c) * fx, bot = px_chan(p10, c) * (32 - fx) + px_chan(p11, c) * fx;
        acc[c] += (top * (32 - fy) + bot * fy + 512) >> 10;
    }
}

template <int SRC, bool F32>
__global__ __launch_bounds__(CR_THREADS) void crop_kernel(const CropArgs p) {
    const int b = blockIdx.z, m = blockIdx.y;
    int n = p.l.count ? p.l.count[(int64_t)b * p.l.count_stride] : p.l.K;
    n = min(n, min(p.l.K, p.M));
    if (m >= n) return;                                                   // not a chip: nothing is written (n <= 0 too)
    // Sampling: lane t computes pixels t, t + 256, ... of the tile's 1024 (the chip's rows, padded to whole groups of 4, laid
    // end to end), so the lanes of a wave sample neighbouring chip pixels and their taps share cache lines.  The packed
    // pixels cross to the store layout -- 4 neighbouring pixels per lane -- through LDS.
    __shared__ __align__(16) uint32_t tile_px[CR_THREADS * 4];
    const int gw = (p.cw + 3) >> 2, rowpx = gw * 4;
    const int first = blockIdx.x * (CR_THREADS * 4), total = p.ch * rowpx;

    const float *bx = p.l.box + (int64_t)b * p.l.box_frame_stride + (int64_t)m * p.l.box_row_stride;
    const float cx = bx[0], cy = bx[1], w = bx[2], h = bx[3];
    const float ang = p.l.angle ? p.l.angle[(int64_t)b * p.l.angle_frame_stride + (int64_t)m * p.l.angle_row_stride] : 0.0f;
    const bool ok = isfinite(cx) && isfinite(cy) && isfinite(w) && isfinite(h) && isfinite(ang) && w > 0.0f && h > 0.0f;
    float c = 1.0f, s = 0.0f;
    if (ok) box_rotation<true>(ang, c, s);
    const float fcw = (float)p.cw, fch = (float)p.ch;
    const float sx = (w * p.pad) / fcw, sy = (h * p.pad) / fch;
    const int nx = (int)fminf(fmaxf(ceilf(sx), 1.0f), 4.0f), ny = (int)fminf(fmaxf(ceilf(sy), 1.0f), 4.0f);
    const int ns = nx * ny;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int e = (int)threadIdx.x + CR_THREADS * k, P = first + e;
        uint32_t v = p.fill;
        const int pi = P / rowpx, pj = P - pi * rowpx;
        if (ok && P < total && pj < p.cw) {
            int acc[3] = {0, 0, 0};
            for (int pp = 0; pp < ny; ++pp) {
                const float ly = ((float)pi + ((float)pp + 0.5f) / (float)ny - 0.5f * fch) * sy;
                for (int q = 0; q < nx; ++q) {
                    const float lx = ((float)pj + ((float)q + 0.5f) / (float)nx - 0.5f * fcw) * sx;
                    const float X = cx + lx * c - ly * s, Y = cy + lx * s + ly * c;
                    crop_sample<SRC>(p, b, X, Y, acc);
                }
            }
            v = px_pack((acc[0] + (ns >> 1)) / ns, (acc[1] + (ns >> 1)) / ns, (acc[2] + (ns >> 1)) / ns);
        }
        tile_px[e] = v;
    }
    __syncthreads();
    const int g = blockIdx.x * CR_THREADS + (int)threadIdx.x;
    if (g >= p.ch * gw) return;
    const int i = g / gw, j0 = (g - i * gw) * 4;
    const int nv = min(4, p.cw - j0);
    const uint4 quad = *reinterpret_cast<const uint4 *>(tile_px + 4 * threadIdx.x);
    const uint32_t px[4] = {quad.x, quad.y, quad.z, quad.w};

    const int64_t base = (int64_t)b * p.frame + (int64_t)m * p.slot;
    if constexpr (F32) {
        float *o = static_cast<float *>(p.out) + base + (int64_t)i * p.cw + j0;
        const int64_t plane = (int64_t)p.ch * p.cw;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float v[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = px_to_float(px_chan(px[k], c), p.norm, p.mean[c], p.sd[c]);
            if (p.wide && nv == 4) {
                *reinterpret_cast<float4 *>(o + c * plane) = make_float4(v[0], v[1], v[2], v[3]);
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (k < nv) o[c * plane + k] = v[k];
            }
        }
    } else {
        unsigned char *o = static_cast<unsigned char *>(p.out) + base + ((int64_t)i * p.cw + j0) * 3;
        if (p.wide && nv == 4) {                                          // 12 bytes at a multiple of 12 from an aligned chip
            uint32_t *o4 = reinterpret_cast<uint32_t *>(o);
            o4[0] = px[0] | (px[1] << 24);
            o4[1] = (px[1] >> 8) | (px[2] << 16);
            o4[2] = (px[2] >> 16) | (px[3] << 8);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k < nv) {
                    o[3 * k] = (unsigned char)px[k]; o[3 * k + 1] = (unsigned char)(px[k] >> 8); o[3 * k + 2] = (unsigned char)(px[k] >> 16);
                }
        }
    }
}

// The checks both entry points share; fills everything of `p` but the source
int crop_setup(CropArgs &p, dim3 &grid, const mydet_draw_list *l, const mydet_crop_out *o, int B, int H, int W) {
    if (!o || B <= 0 || H <= 0 || W <= 0 || paint_list_check(l, false) || o->frame_stride < 0) return MYDET_E_BADARG;
    if (!o->out || o->ch < 1 || o->ch > MYDET_CROP_MAX_SIDE || o->cw < 1 || o->cw > MYDET_CROP_MAX_SIDE) return MYDET_E_BADARG;
    if (o->M < 1 || o->M > MYDET_CROP_MAX_SLOTS) return MYDET_E_BADARG;
    if (!(o->pad > 0.0f) || !(o->pad <= 3.402823466e38f)) return MYDET_E_BADARG;          // NaN, infinity, <= 0
    if (o->kind != MYDET_CROP_U8 && o->kind != MYDET_CROP_F32) return MYDET_E_BADARG;
    if (o->slot_stride < (int64_t)3 * o->ch * o->cw) return MYDET_E_BADARG;
    if (o->norm && (!o->mean3 || !o->std3)) return MYDET_E_BADARG;
    if (B > 65535 || H > (1 << 24) || W > (1 << 24)) return MYDET_E_UNSUPP;
    p.l = *l; p.H = H; p.W = W;
    p.ch = o->ch; p.cw = o->cw; p.M = o->M; p.norm = o->norm != 0; p.pad = o->pad;
    p.fill = (uint32_t)o->fill[0] | ((uint32_t)o->fill[1] << 8) | ((uint32_t)o->fill[2] << 16);
    for (int c = 0; c < 3; ++c) {
        p.mean[c] = p.norm ? o->mean3[c] : 0.0f;
        p.sd[c] = p.norm ? o->std3[c] : 1.0f;
    }
    p.out = o->out; p.slot = o->slot_stride; p.frame = o->frame_stride;
    const uintptr_t mask = o->kind == MYDET_CROP_F32 ? 15 : 3;
    p.wide = o->cw % 4 == 0 && ((uintptr_t)o->out & mask) == 0 && o->slot_stride % 4 == 0 && o->frame_stride % 4 == 0;
    const int groups = o->ch * ((o->cw + 3) / 4);
    grid = dim3((unsigned)((groups + CR_THREADS - 1) / CR_THREADS), (unsigned)o->M, (unsigned)B);
    return 0;
}

template <int SRC>
void crop_launch(const CropArgs &p, const dim3 &grid, int kind, void *stream) {
    if (kind == MYDET_CROP_F32) hipLaunchKernelGGL((crop_kernel<SRC, true>), grid, dim3(CR_THREADS), 0, (hipStream_t)stream, p);
    else hipLaunchKernelGGL((crop_kernel<SRC, false>), grid, dim3(CR_THREADS), 0, (hipStream_t)stream, p);
}

}  // namespace

extern "C" int mydet_crop_boxes_rgb(const unsigned char *src, int B, int H, int W, int64_t src_img_bytes, int64_t src_row_bytes,
                                    const mydet_draw_list *list, const mydet_crop_out *out, void *stream) {
    CropArgs p = {};
    dim3 grid;
    const int code = crop_setup(p, grid, list, out, B, H, W);
    if (code) return code;
    if (!src || src_row_bytes < (int64_t)W * 3 || src_img_bytes < 0) return MYDET_E_BADARG;
    p.src = src; p.img = src_img_bytes; p.row = src_row_bytes;
    crop_launch<0>(p, grid, out->kind, stream);
    return mydet_launch_status();
}

extern "C" int mydet_crop_boxes_yuv420(const mydet_yuv420_src *src, int B, int H, int W, const mydet_draw_list *list,
                                       const mydet_crop_out *out, void *stream) {
    CropArgs p = {};
    dim3 grid;
    int bps;
    bool planar;
    const int source = yuv_source(p.y, bps, planar, src, B, H, W);
    if (source) return source;
    const int code = crop_setup(p, grid, list, out, B, H, W);
    if (code) return code;
#define CROP_YUV(BPS, PLANAR) crop_launch<1 + 2 * (BPS - 1) + (PLANAR ? 1 : 0)>(p, grid, out->kind, stream)
    YUV_DISPATCH(bps, planar, CROP_YUV);
#undef CROP_YUV
    return mydet_launch_status();
}
