// 4:2:0 video frames: a Y plane [H][W] + chroma at half resolution, in the five layouts of include/mydet.h (mydet_yuv420_src):
// NV12 / NV21 / P010 keep (U, V) pairs in one plane [ceil(H/2)][ceil(W/2)][2], I420 / I010 keep a U and a V plane; P010 / I010
// store 16-bit words that are reduced to 8 bits when they are read (yuv_s8).  Every plane has its own row pitch.
//
//   mydet_yuv420_to_rgb_u8     planes -> packed uint8 RGB [B][H][W][3]
//   mydet_yuv420_to_input_f32  planes -> float32 [B,3,Hp,Wp]: the bits mydet_frames_to_input_f32 (frames.hip) gives for the RGB
//                              frames of the conversion below, in one launch, without an RGB image in memory.
//   mydet_nv12_to_rgb_u8, mydet_nv12_to_input_f32: the same two for layout NV12, with the planes as arguments.
//
// Only the fetch of four neighbouring pixels (yuv_quad, templated on bytes per sample and planar / interleaved chroma; the
// V-first order of NV21 is a run-time byte selector) depends on the layout.  Everything behind it works on 8-bit samples.
//
// Conversion (8-bit fixed point, arithmetic shift on int32, nearest-neighbour chroma: pixel (y, x) uses the pair (y >> 1, x >> 1)):
//   C = Y - 16 (limited range) or Y (full range), D = U - 128, E = V - 128
//   R = clip8((cy*C         + crv*E + 128) >> 8)
//   G = clip8((cy*C - cgu*D - cgv*E + 128) >> 8)
//   B = clip8((cy*C + cbu*D         + 128) >> 8)
// with round(256 * x) of the BT.601 / BT.709 matrices in YUV_COEF below, the only copy of the table.
//
// The fused kernel is built from the tile pipeline of frames_tile.h, like frames_to_input_kernel: the same tile, stage of
// horizontally resampled rows, vertical pass and stores, from the same functions.  The horizontal pass differs: the
// taps of neighbouring output columns overlap (7 taps for 3 source pixels per column at 1080p -> 360), so the source is
// converted once per pixel and not once per tap.  YUV_ROWS source rows of the tile's column window [c0, c0 + max_cols) are read
// as quads: a thread fetches four neighbouring pixels from a column that is a multiple of 4 (yuv_quad, where the reads of each
// layout are listed; a wave reads whole row segments), converts them and writes them to LDS as packed dwords
// (r | g << 8 | b << 16) with one 16-byte write.  The taps are then LDS reads (lane stride = the scale factor in dwords), and
// the result goes to the stage.
//
// LDS: (max_rows + ksx) * FR_TW dwords as in frames.hip + YUV_ROWS * max_cols dwords, max_cols <= (FR_TW - 1) * W / ow + ksx + 8:
// at most 39 KiB + 8 * 528 * 4 B = 55.5 KiB at MYDET_FRAMES_MAX_TAPS, 15 + 6.4 KiB for 1080p -> 360 rows.  Every table entry
// is clamped before it addresses either plane or the LDS window, so a malformed table gives wrong pixels, never an access
// outside the planes or the stage.
#include "frames_tile.h"

namespace {

constexpr int YUV_ROWS = 8;                 // source rows converted per step

// cy, crv, cgu, cgv, cbu, luma offset: [matrix: 0 = BT.601, 1 = BT.709][range: 0 = limited, 1 = full]
struct YuvCoef { int cy, crv, cgu, cgv, cbu, yoff; };
constexpr YuvCoef YUV_COEF[2][2] = {{{298, 409, 100, 208, 516, 16}, {256, 359, 88, 183, 454, 0}},
                                    {{298, 459, 55, 136, 541, 16}, {256, 403, 48, 120, 475, 0}}};

// One source of the 4:2:0 family (include/mydet.h: mydet_yuv420_src).  p[2] is null for the semi-planar layouts.
struct YuvSrc {
    const unsigned char *p[3];                 // Y; interleaved chroma or U; V
    int64_t img[3], row[3];                    // bytes between frames / rows of each plane
    int H, W;
    int wide;                                  // every plane allows the wide reads of its layout (yuv_quad)
    uint32_t pair_sel;                         // v_perm_b32 selector that puts the two chroma pairs of a quad into (U, V) order
    YuvCoef k;
};

struct YuvInputArgs {
    YuvSrc s;
    int max_cols;
    FrOut o;
};

struct YuvRgbArgs {
    YuvSrc s;
    unsigned char *dst;
    int64_t dst_img, dst_row;
    int dst_words;                             // dst rows can be written as aligned dwords
};

__device__ __forceinline__ uint32_t yuv_rgb(const YuvCoef &k, int Y, int U, int V) {
    const int c = k.cy * (Y - k.yoff) + 128, d = U - 128, e = V - 128;
    return px_pack(px_clamp((c + k.crv * e) >> 8, 0, 255), px_clamp((c - k.cgu * d - k.cgv * e) >> 8, 0, 255),
                   px_clamp((c + k.cbu * d) >> 8, 0, 255));
}

// A stored sample as 8 bits.  BPS = 2: little-endian words, the ten bits are the high ones of a semi-planar layout (P010) and
// the low ones of a planar layout (I010); the other six are ignored.  s8 = min(255, (v10 + 2) >> 2).
template <int BPS, bool PLANAR>
__device__ __forceinline__ uint32_t yuv_s8(uint32_t w) {
    if constexpr (BPS == 1) {
        return w;
    } else {
        const uint32_t v10 = PLANAR ? (w & 1023u) : ((w & 0xffffu) >> 6);
        return min(255u, (v10 + 2u) >> 2);
    }
}

// N (4 or 2) neighbouring samples from p as packed bytes, sample k in bits [8k, 8k + 8); a sample at or beyond `valid` is zero
// and is not read.  One N * BPS byte read when `wide` (p is then a multiple of N * BPS) and all N are valid, else by samples.
template <int BPS, bool PLANAR, int N>
__device__ __forceinline__ uint32_t yuv_samples(const unsigned char *p, int valid, int wide) {
    uint32_t v = 0;
    if (wide && valid >= N) {
        if constexpr (BPS == 1 && N == 4) {
            v = *reinterpret_cast<const uint32_t *>(p);
        } else if constexpr (BPS == 1) {
            v = *reinterpret_cast<const uint16_t *>(p);
        } else if constexpr (N == 4) {
            const uint2 t = *reinterpret_cast<const uint2 *>(p);
            v = yuv_s8<BPS, PLANAR>(t.x & 0xffffu) | (yuv_s8<BPS, PLANAR>(t.x >> 16) << 8) |
                (yuv_s8<BPS, PLANAR>(t.y & 0xffffu) << 16) | (yuv_s8<BPS, PLANAR>(t.y >> 16) << 24);
        } else {
            const uint32_t t = *reinterpret_cast<const uint32_t *>(p);
            v = yuv_s8<BPS, PLANAR>(t & 0xffffu) | (yuv_s8<BPS, PLANAR>(t >> 16) << 8);
        }
    } else {
#pragma unroll
        for (int k = 0; k < N; ++k)
            if (k < valid) {
                uint32_t t;
                if constexpr (BPS == 1) t = p[k];
                else t = reinterpret_cast<const uint16_t *>(p)[k];
                v |= yuv_s8<BPS, PLANAR>(t) << (8 * k);
            }
    }
    return v;
}

// Four neighbouring pixels of source row `row` of frame `b` from column c (c % 4 == 0) as packed dwords; a pixel at or beyond W
// is zero.  The only code that depends on the layout.  A Y row holds W samples; an interleaved chroma row 2 * ceil(W / 2), the
// pair of pixel c + k starting at sample c + (k & ~1); a planar chroma row ceil(W / 2), the sample of pixel c + k at (c + k) >> 1.
// Wide reads per quad, taken when the address, pitch and frame stride of every plane are multiples of the bytes read there:
//   NV12 / NV21  Y 4 bytes, chroma 4 bytes at byte c                      every plane: 4
//   I420         Y 4 bytes, U and V 2 bytes at byte c / 2                 Y: 4, U and V: 2
//   P010         Y 8 bytes, chroma 8 bytes at byte 2c                     every plane: 8
//   I010         Y 8 bytes, U and V 4 bytes at byte c                     Y: 8, U and V: 4
// Otherwise, and in a row's partial last quad, the samples are read one by one (the 16-bit layouts need even addresses: the
// entry points refuse anything else).
template <int BPS, bool PLANAR>
__device__ __forceinline__ uint4 yuv_quad(const YuvSrc &s, int b, int row, int c) {
    const unsigned char *yr = s.p[0] + (int64_t)b * s.img[0] + (int64_t)row * s.row[0] + c * BPS;
    const unsigned char *ur = s.p[1] + (int64_t)b * s.img[1] + (int64_t)(row >> 1) * s.row[1];
    const int ny = s.W - c;                                             // valid samples from c on
    const uint32_t yw = yuv_samples<BPS, PLANAR, 4>(yr, ny, s.wide);
    uint32_t cw;                                                        // the two pairs: bytes (first, second) x 2
    if constexpr (PLANAR) {
        const unsigned char *vr = s.p[2] + (int64_t)b * s.img[2] + (int64_t)(row >> 1) * s.row[2];
        const int nc = ((s.W + 1) >> 1) - (c >> 1);
        const uint32_t u = yuv_samples<BPS, PLANAR, 2>(ur + (c >> 1) * BPS, nc, s.wide);
        const uint32_t v = yuv_samples<BPS, PLANAR, 2>(vr + (c >> 1) * BPS, nc, s.wide);
        cw = (u & 255u) | ((v & 255u) << 8) | ((u >> 8) << 16) | ((v >> 8) << 24);
    } else {
        cw = yuv_samples<BPS, PLANAR, 4>(ur + c * BPS, ((s.W + 1) & ~1) - c, s.wide);
        cw = __builtin_amdgcn_perm(cw, cw, s.pair_sel);                 // NV21: (V, U) -> (U, V); the identity otherwise
    }
    uint32_t v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t pair = cw >> (16 * (k >> 1));
        v[k] = k < ny ? yuv_rgb(s.k, (yw >> (8 * k)) & 255u, pair & 255u, (pair >> 8) & 255u) : 0u;
    }
    return make_uint4(v[0], v[1], v[2], v[3]);
}

// 64 quads x 4 rows per workgroup
template <int BPS, bool PLANAR>
__global__ __launch_bounds__(256) void yuv_to_rgb_kernel(const YuvRgbArgs p) {
    const int c = (blockIdx.x * 64 + (threadIdx.x & 63)) * 4, row = blockIdx.y * 4 + (threadIdx.x >> 6), b = blockIdx.z;
    if (c >= p.s.W || row >= p.s.H) return;
    const uint4 v = yuv_quad<BPS, PLANAR>(p.s, b, row, c);
    unsigned char *o = p.dst + (int64_t)b * p.dst_img + (int64_t)row * p.dst_row + (int64_t)c * 3;
    if (p.dst_words && c + 4 <= p.s.W) {                                // 12 bytes at a multiple of 12
        uint32_t *o4 = reinterpret_cast<uint32_t *>(o);
        o4[0] = v.x | (v.y << 24);
        o4[1] = (v.y >> 8) | (v.z << 16);
        o4[2] = (v.z >> 16) | (v.w << 8);
    } else {
        const uint32_t q[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (c + k < p.s.W) {
                o[3 * k] = (unsigned char)q[k]; o[3 * k + 1] = (unsigned char)(q[k] >> 8); o[3 * k + 2] = (unsigned char)(q[k] >> 16);
            }
    }
}

// N = pixels per thread along x of the vertical pass and the stores: 4 or 1 (frames_tile.h); BPS, PLANAR: the fetch (yuv_quad)
template <int N, int BPS, bool PLANAR>
__global__ __launch_bounds__(256) void yuv_to_input_kernel(const YuvInputArgs p) {
    extern __shared__ __align__(16) uint32_t yuv_lds[];
    uint32_t *stage = yuv_lds;                                           // [max_rows][FR_TW] horizontally resampled pixels
    int32_t *wts = reinterpret_cast<int32_t *>(yuv_lds + p.o.max_rows * FR_TW);   // [ksx][FR_TW] horizontal weights, tap-major
    uint32_t *raw = yuv_lds + (p.o.max_rows + p.o.ksx) * FR_TW;          // [YUV_ROWS][max_cols] converted source pixels
    const int tid = threadIdx.x;
    const int tx0 = blockIdx.x * FR_TW, ty0 = blockIdx.y * FR_TH, b = blockIdx.z;

    const FrWindow win = fr_window(p.o, p.s.H, tx0, ty0);
    if (win.live) {
        // first column of the window, on a quad: the first tap of the tile's first column (taps start in column order)
        const int c0 = px_clamp(p.o.bx ? p.o.bx[2 * win.wx_lo] : win.wx_lo, 0, p.s.W - 1) & ~3;
        if (p.o.bx) fr_stage_weights(p.o, wts, tx0, tid);               // read after the first barrier below
        // a thread owns one column of the tile: its taps are raw[xs, xs + nx)
        const int col = tid & (FR_TW - 1), wv = tid >> 6;
        const FrColumn c = fr_column(p.o, p.s.W, tx0, col);
        const int xs = px_clamp(c.x0 - c0, 0, p.max_cols - 1), nx = min(c.nx, p.max_cols - xs);
        const int nq = p.max_cols >> 2;
        for (int rb = 0; rb < win.nrows; rb += YUV_ROWS) {
            const int nr = min(YUV_ROWS, win.nrows - rb);
            if (rb) __syncthreads();                                    // the previous step's taps have been read
            for (int r = wv; r < nr; r += 256 / FR_TW)                  // a wave converts a row of the window
                for (int q = col; q < nq; q += FR_TW)
                    *reinterpret_cast<uint4 *>(raw + r * p.max_cols + 4 * q) = yuv_quad<BPS, PLANAR>(p.s, b, win.r0 + rb + r, c0 + 4 * q);
            __syncthreads();
            for (int r = wv; r < nr; r += 256 / FR_TW) {                // horizontal pass
                uint32_t v = 0;
                if (c.inside) {
                    const uint32_t *px = raw + r * p.max_cols + xs;
                    if (p.o.bx) {
                        PxFilter f;
                        for (int t = 0; t < nx; ++t) f.add(px[t], wts[t * FR_TW + col]);
                        v = f.pixel();
                    } else {
                        v = px[0];
                    }
                }
                stage[(rb + r) * FR_TW + col] = v;
            }
        }
    }
    __syncthreads();
    fr_vertical_store<N>(p.o, stage, win, tx0, ty0, b, tid);
}

// bytes per sample and plane count of a layout selector; false for an unknown one
inline bool yuv_layout(int layout, int &bps, bool &planar, bool &v_first) {
    switch (layout) {
    case MYDET_YUV420_NV12: bps = 1; planar = false; v_first = false; return true;
    case MYDET_YUV420_NV21: bps = 1; planar = false; v_first = true; return true;
    case MYDET_YUV420_I420: bps = 1; planar = true; v_first = false; return true;
    case MYDET_YUV420_P010: bps = 2; planar = false; v_first = false; return true;
    case MYDET_YUV420_I010: bps = 2; planar = true; v_first = false; return true;
    }
    return false;
}

// The checks every entry point shares; fills `s`, `bps` and `planar`
int yuv_source(YuvSrc &s, int &bps, bool &planar, const mydet_yuv420_src *src, int B, int H, int W) {
    bool v_first;
    if (!src || !src->plane[0] || !src->plane[1] || B <= 0 || H <= 0 || W <= 0) return MYDET_E_BADARG;
    if (!yuv_layout(src->layout, bps, planar, v_first)) return MYDET_E_BADARG;
    if (src->matrix < 0 || src->matrix > 1 || src->full_range < 0 || src->full_range > 1) return MYDET_E_BADARG;
    if ((src->plane[2] != nullptr) != planar) return MYDET_E_BADARG;
    const int64_t cw = ((int64_t)W + 1) / 2;
    const int64_t need[3] = {(int64_t)W * bps, (planar ? cw : 2 * cw) * bps, cw * bps};
    const int wide[3] = {4 * bps, planar ? 2 * bps : 4 * bps, 2 * bps};           // bytes of a plane's wide read (yuv_quad)
    s.wide = 1;
    for (int i = 0; i < (planar ? 3 : 2); ++i) {
        if (src->row_bytes[i] < need[i] || src->img_bytes[i] < 0) return MYDET_E_BADARG;
        const uintptr_t bits = (uintptr_t)src->plane[i] | (uintptr_t)src->row_bytes[i] | (uintptr_t)src->img_bytes[i];
        if (bits & (uintptr_t)(bps - 1)) return MYDET_E_BADARG;                   // a 16-bit sample at an odd address
        if (bits & (uintptr_t)(wide[i] - 1)) s.wide = 0;
    }
    for (int i = 0; i < 3; ++i) {
        const bool used = i < 2 || planar;
        s.p[i] = used ? static_cast<const unsigned char *>(src->plane[i]) : nullptr;
        s.img[i] = used ? src->img_bytes[i] : 0;
        s.row[i] = used ? src->row_bytes[i] : 0;
    }
    s.H = H; s.W = W;
    s.pair_sel = v_first ? 0x02030001u : 0x03020100u;
    s.k = YUV_COEF[src->matrix][src->full_range];
    return 0;
}

// CALL(BPS, PLANAR) for the layout's instance
#define YUV_DISPATCH(bps, planar, CALL)                    \
    do {                                                   \
        if ((bps) == 1 && !(planar)) { CALL(1, false); }   \
        else if ((bps) == 1) { CALL(1, true); }            \
        else if (!(planar)) { CALL(2, false); }            \
        else { CALL(2, true); }                            \
    } while (0)

// The NV12 entry points' arguments as a source descriptor
mydet_yuv420_src nv12_src(const unsigned char *y, int64_t y_img, int64_t y_row, const unsigned char *uv, int64_t uv_img, int64_t uv_row,
                          int matrix, int full_range) {
    return {{y, uv, nullptr}, {y_img, uv_img, 0}, {y_row, uv_row, 0}, MYDET_YUV420_NV12, matrix, full_range, 0};
}

}  // namespace

extern "C" int mydet_yuv420_to_rgb_u8(const mydet_yuv420_src *src, int B, int H, int W, unsigned char *dst, int64_t dst_img_bytes,
                                      int64_t dst_row_bytes, void *stream) {
    YuvRgbArgs p;
    int bps;
    bool planar;
    const int code = yuv_source(p.s, bps, planar, src, B, H, W);
    if (code) return code;
    if (!dst || dst_row_bytes < (int64_t)W * 3 || dst_img_bytes < 0) return MYDET_E_BADARG;
    const int gy = (H + 3) / 4;
    if (B > 65535 || gy > 65535) return MYDET_E_UNSUPP;
    p.dst = dst; p.dst_img = dst_img_bytes; p.dst_row = dst_row_bytes;
    p.dst_words = (((uintptr_t)dst | (uintptr_t)dst_img_bytes | (uintptr_t)dst_row_bytes) & 3) == 0;
    const dim3 grid((unsigned)((W + 255) / 256), (unsigned)gy, (unsigned)B);
#define YUV_RGB(BPS, PLANAR) hipLaunchKernelGGL((yuv_to_rgb_kernel<BPS, PLANAR>), grid, dim3(256), 0, (hipStream_t)stream, p)
    YUV_DISPATCH(bps, planar, YUV_RGB);
#undef YUV_RGB
    return mydet_launch_status();
}

extern "C" int mydet_yuv420_to_input_f32(const mydet_yuv420_src *src, int B, int H, int W, float *out, int Hp, int Wp, int oh, int ow,
                                         int top, int left, const int32_t *bounds_x, const int32_t *kx, int ksx,
                                         const int32_t *bounds_y, const int32_t *ky, int ksy, int norm, const float *mean3,
                                         const float *std3, void *stream) {
    YuvInputArgs p;
    int bps;
    bool planar;
    const int code = yuv_source(p.s, bps, planar, src, B, H, W);
    if (code) return code;
    dim3 grid;
    const int tile = fr_tile_setup(p.o, grid, B, H, W, out, Hp, Wp, oh, ow, top, left, bounds_x, kx, ksx, bounds_y, ky, ksy, norm,
                                   mean3, std3);
    if (tile) return tile;
    // source columns under FR_TW output columns, by the rule of max_rows (frames_tile.h): <= (FR_TW - 1) * scale + ksx, + 2 spare.
    // The column window starts on a quad (+ 3) and is a whole number of quads.  It holds converted pixels: the same for every layout.
    int64_t cols = FR_TW;
    if (bounds_x) cols = (int64_t)((double)(FR_TW - 1) * (double)W / (double)ow) + ksx + 2;
    cols = (cols + 3 + 3) / 4 * 4;
    if (cols > ((int64_t)W + 3) / 4 * 4) cols = ((int64_t)W + 3) / 4 * 4;
    p.max_cols = (int)cols;
    const size_t lds = fr_tile_lds_bytes(p.o) + (size_t)YUV_ROWS * p.max_cols * sizeof(uint32_t);
    if (lds > 64 * 1024) return MYDET_E_UNSUPP;
    const bool quads = fr_quad_stores(p.o);
#define YUV_INPUT(BPS, PLANAR)                                                                                          \
    if (quads) hipLaunchKernelGGL((yuv_to_input_kernel<4, BPS, PLANAR>), grid, dim3(256), lds, (hipStream_t)stream, p); \
    else hipLaunchKernelGGL((yuv_to_input_kernel<1, BPS, PLANAR>), grid, dim3(256), lds, (hipStream_t)stream, p)
    YUV_DISPATCH(bps, planar, YUV_INPUT);
#undef YUV_INPUT
    return mydet_launch_status();
}

extern "C" int mydet_nv12_to_rgb_u8(const unsigned char *y, int64_t y_img_bytes, int64_t y_row_bytes, const unsigned char *uv,
                                    int64_t uv_img_bytes, int64_t uv_row_bytes, int B, int H, int W, unsigned char *dst,
                                    int64_t dst_img_bytes, int64_t dst_row_bytes, int matrix, int full_range, void *stream) {
    const mydet_yuv420_src src = nv12_src(y, y_img_bytes, y_row_bytes, uv, uv_img_bytes, uv_row_bytes, matrix, full_range);
    return mydet_yuv420_to_rgb_u8(&src, B, H, W, dst, dst_img_bytes, dst_row_bytes, stream);
}

extern "C" int mydet_nv12_to_input_f32(const unsigned char *y, int64_t y_img_bytes, int64_t y_row_bytes, const unsigned char *uv,
                                       int64_t uv_img_bytes, int64_t uv_row_bytes, int B, int H, int W, int matrix, int full_range,
                                       float *out, int Hp, int Wp, int oh, int ow, int top, int left, const int32_t *bounds_x,
                                       const int32_t *kx, int ksx, const int32_t *bounds_y, const int32_t *ky, int ksy, int norm,
                                       const float *mean3, const float *std3, void *stream) {
    const mydet_yuv420_src src = nv12_src(y, y_img_bytes, y_row_bytes, uv, uv_img_bytes, uv_row_bytes, matrix, full_range);
    return mydet_yuv420_to_input_f32(&src, B, H, W, out, Hp, Wp, oh, ow, top, left, bounds_x, kx, ksx, bounds_y, ky, ksy, norm, mean3, std3,
                                     stream);
}
