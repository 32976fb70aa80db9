// Video frames -> network input in one launch: B uint8 HWC frames of ONE size -> float32 [B,3,Hp,Wp].
//
//   Pillow's bilinear resize to oh x ow (the two-pass 8-bit fixed-point filter of boxops.hip: horizontal pass rounded to
//   uint8, vertical pass on those uint8 values), placed at (top, left) of a zero image of Hp x Wp, then x / 255 and, with
//   norm, (x - mean[c]) / std[c] in the operation order of preprocess_kernel (boxops.hip) -- the floats are the ones
//   mydet_resize_bilinear_u8 + mydet_preprocess_u8_f32 produce, bit for bit, without the uint8 image in between.  The
//   filter rounding and the float conversion are the same functions those kernels call (pixel_math.h).
//
// The tile, the stage of horizontally resampled rows, the vertical pass and the stores are frames_tile.h, shared with
// yuv420.hip; this file is the horizontal pass over packed RGB bytes in global memory and the entry point.
//
// LDS: (rows + ksx) * FR_TW dwords, rows <= (FR_TH - 1) * H / oh + ksy + 2.  With MYDET_FRAMES_MAX_TAPS = 17 (a downscale
// of up to 8x: ksize = 2 * ceil(scale) + 1) that is at most 139 + 17 rows of 256 bytes = 39 KiB, and 53 + 7 rows (15 KiB)
// for 1080p -> 360 rows: several workgroups per CU, no opt-in.
#include "frames_tile.h"

namespace {

struct FramesArgs {
    const unsigned char *src;
    int64_t src_img, src_row;                  // bytes between frames / rows
    int H, W;
    int flip;                                  // MYDET_VIEW_* bits; read by the FLIP instances only
    FrOut o;
};

// N = pixels per thread along x of the vertical pass and the stores: 4 or 1 (frames_tile.h).  FLIP: the mirrored views
// (frames_tile.h); the <N, false> instances are the ones mydet_frames_to_input_f32 has always launched.
template <int N, bool FLIP>
__global__ __launch_bounds__(256) void frames_to_input_kernel(const FramesArgs p) {
    extern __shared__ __align__(16) uint32_t fr_lds[];
    uint32_t *stage = fr_lds;                                           // [max_rows][FR_TW] packed pixels
    int32_t *wts = reinterpret_cast<int32_t *>(fr_lds + p.o.max_rows * FR_TW);   // [ksx][FR_TW] horizontal weights, tap-major
    const int tid = threadIdx.x;
    const int tx0 = blockIdx.x * FR_TW, ty0 = blockIdx.y * FR_TH, b = blockIdx.z;
    const unsigned char *src = p.src + (int64_t)b * p.src_img;

    const FrWindow win = fr_window(p.o, p.H, tx0, ty0);
    if (win.live) {
        if (p.o.bx) {
            fr_stage_weights(p.o, wts, tx0, tid);
            __syncthreads();
        }
        // horizontal pass: a thread owns one column of the tile and every fourth source row
        const int col = tid & (FR_TW - 1);
        const FrColumn c = fr_column(p.o, p.W, tx0, col);
        for (int r = tid >> 6; r < win.nrows; r += 256 / FR_TW) {
            uint32_t v = 0;
            if (c.inside) {
                // tap t is `step` * t bytes from the first one: backwards in a horizontally mirrored view
                int64_t row = win.r0 + r;
                int x = c.x0, step = 3;
                if constexpr (FLIP) {
                    row = fr_src_row(p.flip, p.H, win.r0 + r);
                    x = fr_src_col(p.flip, p.W, c.x0);
                    step = (p.flip & MYDET_VIEW_HFLIP) ? -3 : 3;
                }
                const unsigned char *px = src + row * p.src_row + x * 3;
                if (p.o.bx) {
                    PxFilter f;
                    for (int t = 0; t < c.nx; ++t) f.add(px[step * t], px[step * t + 1], px[step * t + 2], wts[t * FR_TW + col]);
                    v = f.pixel();
                } else {
                    v = px_pack(px[0], px[1], px[2]);
                }
            }
            stage[r * FR_TW + col] = v;
        }
    }
    __syncthreads();
    fr_vertical_store<N>(p.o, stage, win, tx0, ty0, b, tid);
}

}  // namespace

// flip == 0 launches the <N, false> instances: the launch mydet_frames_to_input_f32 has always made
static int frames_to_input(const unsigned char *src, int B, int H, int W, int64_t src_img_bytes, int64_t src_row_bytes, float *out,
                           int Hp, int Wp, int oh, int ow, int top, int left, const int32_t *bounds_x, const int32_t *kx, int ksx,
                           const int32_t *bounds_y, const int32_t *ky, int ksy, int norm, const float *mean3, const float *std3,
                           int flip, void *stream) {
    if (!src || B <= 0 || H <= 0 || W <= 0 || src_row_bytes < (int64_t)W * 3 || src_img_bytes < 0) return MYDET_E_BADARG;
    if (fr_flip_arg(flip)) return MYDET_E_BADARG;
    FramesArgs p;
    dim3 grid;
    const int code = fr_tile_setup(p.o, grid, B, H, W, out, Hp, Wp, oh, ow, top, left, bounds_x, kx, ksx, bounds_y, ky, ksy, norm,
                                   mean3, std3);
    if (code) return code;
    p.src = src; p.src_img = src_img_bytes; p.src_row = src_row_bytes; p.H = H; p.W = W; p.flip = flip;
    const size_t lds = fr_tile_lds_bytes(p.o);
    if (lds > 64 * 1024) return MYDET_E_UNSUPP;
    const bool quads = fr_quad_stores(p.o);
    if (flip) {
        if (quads) hipLaunchKernelGGL((frames_to_input_kernel<4, true>), grid, dim3(256), lds, (hipStream_t)stream, p);
        else hipLaunchKernelGGL((frames_to_input_kernel<1, true>), grid, dim3(256), lds, (hipStream_t)stream, p);
    } else if (quads) {
        hipLaunchKernelGGL((frames_to_input_kernel<4, false>), grid, dim3(256), lds, (hipStream_t)stream, p);
    } else {
        hipLaunchKernelGGL((frames_to_input_kernel<1, false>), grid, dim3(256), lds, (hipStream_t)stream, p);
    }
    return mydet_launch_status();
}

extern "C" int mydet_frames_to_input_f32(const unsigned char *src, int B, int H, int W, int64_t src_img_bytes,
                                         int64_t src_row_bytes, float *out, int Hp, int Wp, int oh, int ow, int top, int left,
                                         const int32_t *bounds_x, const int32_t *kx, int ksx, const int32_t *bounds_y,
                                         const int32_t *ky, int ksy, int norm, const float *mean3, const float *std3,
                                         void *stream) {
    return frames_to_input(src, B, H, W, src_img_bytes, src_row_bytes, out, Hp, Wp, oh, ow, top, left, bounds_x, kx, ksx, bounds_y, ky,
                           ksy, norm, mean3, std3, 0, stream);
}

extern "C" int mydet_frames_to_input_flip_f32(const unsigned char *src, int B, int H, int W, int64_t src_img_bytes,
                                              int64_t src_row_bytes, float *out, int Hp, int Wp, int oh, int ow, int top, int left,
                                              const int32_t *bounds_x, const int32_t *kx, int ksx, const int32_t *bounds_y,
                                              const int32_t *ky, int ksy, int norm, const float *mean3, const float *std3,
                                              int flip, void *stream) {
    return frames_to_input(src, B, H, W, src_img_bytes, src_row_bytes, out, Hp, Wp, oh, ow, top, left, bounds_x, kx, ksx, bounds_y, ky,
                           ksy, norm, mean3, std3, flip, stream);
}
