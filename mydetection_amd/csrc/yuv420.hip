// 4:2:0 video frames: a Y plane [H][W] + chroma at half resolution, in the five layouts of include/mydet.h (mydet_yuv420_src):
// NV12 / NV21 / P010 keep (U, V) pairs in one plane [ceil(H/2)][ceil(W/2)][2], I420 / I010 keep a U and a V plane; P010 / I010
// store 16-bit words that are reduced to 8 bits when they are read (yuv_s8).  Every plane has its own row pitch.
//
//   mydet_yuv420_to_rgb_u8     planes -> packed uint8 RGB [B][H][W][3]
//   mydet_yuv420_to_input_f32  planes -> float32 [B,3,Hp,Wp]: the bits mydet_frames_to_input_f32 (frames.hip) gives for the RGB
//                              frames of the conversion below, in one launch, without an RGB image in memory.
//   mydet_nv12_to_rgb_u8, mydet_nv12_to_input_f32: the same two for layout NV12, with the planes as arguments.
//
// Only the fetch of four neighbouring pixels (yuv_quad in yuv_fetch.h, which crop.hip shares; templated on bytes per sample and
// planar / interleaved chroma; the V-first order of NV21 is a run-time byte selector) depends on the layout.  Everything behind
// it works on 8-bit samples.
//
// Conversion (8-bit fixed point, arithmetic shift on int32, nearest-neighbour chroma: pixel (y, x) uses the pair (y >> 1, x >> 1)):
//   C = Y - 16 (limited range) or Y (full range), D = U - 128, E = V - 128
//   R = clip8((cy*C         + crv*E + 128) >> 8)
//   G = clip8((cy*C - cgu*D - cgv*E + 128) >> 8)
//   B = clip8((cy*C + cbu*D         + 128) >> 8)
// with round(256 * x) of the BT.601 / BT.709 matrices in YUV_COEF (yuv_fetch.h), the only copy of the table.
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
#include "yuv_fetch.h"

namespace {

constexpr int YUV_ROWS = 8;                 // source rows converted per step

struct YuvInputArgs {
    YuvSrc s;
    int max_cols;
    int flip;                                  // MYDET_VIEW_* bits; read by the FLIP instances only
    FrOut o;
};

struct YuvRgbArgs {
    YuvSrc s;
    unsigned char *dst;
    int64_t dst_img, dst_row;
    int dst_words;                             // dst rows can be written as aligned dwords
};

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

// N = pixels per thread along x of the vertical pass and the stores: 4 or 1 (frames_tile.h); BPS, PLANAR: the fetch (yuv_quad).
// FLIP: the mirrored views (frames_tile.h).  `raw` keeps the columns of the MIRRORED frame, so the horizontal pass is unchanged;
// the fetch reads row fr_src_row and, when mirrored horizontally, the quad of the frame in memory that holds the four mirrored
// columns and writes it reversed.  For that the window starts where W - c0 is a multiple of 4 (c0 >= -3: mirrored columns below 0
// are columns >= W in memory, which yuv_quad gives as zero without reading), and a quad that would start below column 0 is
// zero.  Luma and chroma are both fetched for the pixel's position in memory, so odd W and H need no rule of their own.
template <int N, int BPS, bool PLANAR, bool FLIP>
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
        int c0 = px_clamp(p.o.bx ? p.o.bx[2 * win.wx_lo] : win.wx_lo, 0, p.s.W - 1);
        bool hflip = false;
        if constexpr (FLIP) hflip = (p.flip & MYDET_VIEW_HFLIP) != 0;
        c0 = hflip ? p.s.W - ((p.s.W - c0 + 3) & ~3) : c0 & ~3;
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
                for (int q = col; q < nq; q += FR_TW) {
                    uint4 v;
                    if constexpr (FLIP) {
                        const int row = fr_src_row(p.flip, p.s.H, win.r0 + rb + r);
                        if (hflip) {
                            const int a = p.s.W - c0 - 4 * (q + 1);     // mirrored columns c0 + 4q + 3 .. c0 + 4q, a multiple of 4
                            v = make_uint4(0u, 0u, 0u, 0u);
                            if (a >= 0) {
                                const uint4 t = yuv_quad<BPS, PLANAR>(p.s, b, row, a);
                                v = make_uint4(t.w, t.z, t.y, t.x);
                            }
                        } else {
                            v = yuv_quad<BPS, PLANAR>(p.s, b, row, c0 + 4 * q);
                        }
                    } else {
                        v = yuv_quad<BPS, PLANAR>(p.s, b, win.r0 + rb + r, c0 + 4 * q);
                    }
                    *reinterpret_cast<uint4 *>(raw + r * p.max_cols + 4 * q) = v;
                }
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

// flip == 0 launches the <N, BPS, PLANAR, false> instances: the launch mydet_yuv420_to_input_f32 has always made
static int yuv420_to_input(const mydet_yuv420_src *src, int B, int H, int W, float *out, int Hp, int Wp, int oh, int ow, int top, int left,
                           const int32_t *bounds_x, const int32_t *kx, int ksx, const int32_t *bounds_y, const int32_t *ky, int ksy,
                           int norm, const float *mean3, const float *std3, int flip, void *stream) {
    if (fr_flip_arg(flip)) return MYDET_E_BADARG;
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
    p.flip = flip;
    const size_t lds = fr_tile_lds_bytes(p.o) + (size_t)YUV_ROWS * p.max_cols * sizeof(uint32_t);
    if (lds > 64 * 1024) return MYDET_E_UNSUPP;
    const bool quads = fr_quad_stores(p.o);
#define YUV_INPUT_F(BPS, PLANAR, FLIP)                                                                                        \
    if (quads) hipLaunchKernelGGL((yuv_to_input_kernel<4, BPS, PLANAR, FLIP>), grid, dim3(256), lds, (hipStream_t)stream, p); \
    else hipLaunchKernelGGL((yuv_to_input_kernel<1, BPS, PLANAR, FLIP>), grid, dim3(256), lds, (hipStream_t)stream, p)
#define YUV_INPUT(BPS, PLANAR) YUV_INPUT_F(BPS, PLANAR, false)
#define YUV_INPUT_FLIP(BPS, PLANAR) YUV_INPUT_F(BPS, PLANAR, true)
    if (flip) YUV_DISPATCH(bps, planar, YUV_INPUT_FLIP);
    else YUV_DISPATCH(bps, planar, YUV_INPUT);
#undef YUV_INPUT_FLIP
#undef YUV_INPUT
#undef YUV_INPUT_F
    return mydet_launch_status();
}

extern "C" int mydet_yuv420_to_input_f32(const mydet_yuv420_src *src, int B, int H, int W, float *out, int Hp, int Wp, int oh, int ow,
                                         int top, int left, const int32_t *bounds_x, const int32_t *kx, int ksx,
                                         const int32_t *bounds_y, const int32_t *ky, int ksy, int norm, const float *mean3,
                                         const float *std3, void *stream) {
    return yuv420_to_input(src, B, H, W, out, Hp, Wp, oh, ow, top, left, bounds_x, kx, ksx, bounds_y, ky, ksy, norm, mean3, std3, 0, stream);
}

extern "C" int mydet_yuv420_to_input_flip_f32(const mydet_yuv420_src *src, int B, int H, int W, float *out, int Hp, int Wp, int oh,
                                              int ow, int top, int left, const int32_t *bounds_x, const int32_t *kx, int ksx,
                                              const int32_t *bounds_y, const int32_t *ky, int ksy, int norm, const float *mean3,
                                              const float *std3, int flip, void *stream) {
    return yuv420_to_input(src, B, H, W, out, Hp, Wp, oh, ow, top, left, bounds_x, kx, ksx, bounds_y, ky, ksy, norm, mean3, std3, flip,
                           stream);
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
