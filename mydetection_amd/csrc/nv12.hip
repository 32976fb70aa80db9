// NV12 video frames: Y plane [H][W] + interleaved chroma plane [ceil(H/2)][ceil(W/2)] (U, V), each with its own row pitch.
//
//   mydet_nv12_to_rgb_u8     NV12 -> packed uint8 RGB [B][H][W][3]
//   mydet_nv12_to_input_f32  NV12 -> float32 [B,3,Hp,Wp]: the bits mydet_frames_to_input_f32 (frames.hip) gives for the RGB
//                            frames of the conversion below, in one launch, without an RGB image in memory.
//
// Conversion (8-bit fixed point, arithmetic shift on int32, nearest-neighbour chroma: pixel (y, x) uses the pair (y >> 1, x >> 1)):
//   C = Y - 16 (limited range) or Y (full range), D = U - 128, E = V - 128
//   R = clip8((cy*C         + crv*E + 128) >> 8)
//   G = clip8((cy*C - cgu*D - cgv*E + 128) >> 8)
//   B = clip8((cy*C + cbu*D         + 128) >> 8)
// with round(256 * x) of the BT.601 / BT.709 matrices in NV_COEF below, the only copy of the table.
//
// The fused kernel is built from the tile pipeline of frames_tile.h, like frames_to_input_kernel: the same tile, stage of
// horizontally resampled rows, vertical pass and stores, from the same functions.  The horizontal pass differs: the
// taps of neighbouring output columns overlap (7 taps for 3 source pixels per column at 1080p -> 360), so the source is
// converted once per pixel and not once per tap.  NV_ROWS source rows of the tile's column window [c0, c0 + max_cols) are read
// as quads -- one Y dword and one chroma dword per thread (a quad starts at a multiple of 4, so both are at byte c of their
// rows), a wave reads whole row segments -- converted, and written to LDS as packed dwords (r | g << 8 | b << 16) with one
// 16-byte write.  The taps are then LDS reads (lane stride = the scale factor in dwords), and the result goes to the stage.
//
// LDS: (max_rows + ksx) * FR_TW dwords as in frames.hip + NV_ROWS * max_cols dwords, max_cols <= (FR_TW - 1) * W / ow + ksx + 8:
// at most 39 KiB + 8 * 528 * 4 B = 55.5 KiB at MYDET_FRAMES_MAX_TAPS, 15 + 6.4 KiB for 1080p -> 360 rows.  Every table entry
// is clamped before it addresses either plane or the LDS window, so a malformed table gives wrong pixels, never an access
// outside the planes or the stage.
#include "frames_tile.h"

namespace {

constexpr int NV_ROWS = 8;                 // source rows converted per step

// cy, crv, cgu, cgv, cbu, luma offset: [matrix: 0 = BT.601, 1 = BT.709][range: 0 = limited, 1 = full]
struct Nv12Coef { int cy, crv, cgu, cgv, cbu, yoff; };
constexpr Nv12Coef NV_COEF[2][2] = {{{298, 409, 100, 208, 516, 16}, {256, 359, 88, 183, 454, 0}},
                                    {{298, 459, 55, 136, 541, 16}, {256, 403, 48, 120, 475, 0}}};

struct Nv12Src {
    const unsigned char *y, *uv;
    int64_t y_img, y_row, uv_img, uv_row;      // bytes between frames / rows of each plane
    int H, W;
    int words;                                 // both planes can be read as aligned dwords
    Nv12Coef k;
};

struct Nv12InputArgs {
    Nv12Src s;
    int max_cols;
    FrOut o;
};

struct Nv12RgbArgs {
    Nv12Src s;
    unsigned char *dst;
    int64_t dst_img, dst_row;
    int dst_words;                             // dst rows can be written as aligned dwords
};

__device__ __forceinline__ uint32_t nv_rgb(const Nv12Coef &k, int Y, int U, int V) {
    const int c = k.cy * (Y - k.yoff) + 128, d = U - 128, e = V - 128;
    return px_pack(px_clamp((c + k.crv * e) >> 8, 0, 255), px_clamp((c - k.cgu * d - k.cgv * e) >> 8, 0, 255),
                   px_clamp((c + k.cbu * d) >> 8, 0, 255));
}

// Four neighbouring pixels of source row `row` from column c (c % 4 == 0) as packed dwords; a pixel at or beyond W is zero.
// The chroma row holds 2 * ceil(W / 2) bytes; the pair of pixel c + k starts at byte c + (k & ~1).
__device__ __forceinline__ uint4 nv_quad(const Nv12Src &s, const unsigned char *y, const unsigned char *uv, int row, int c) {
    const unsigned char *yr = y + (int64_t)row * s.y_row + c;
    const unsigned char *cr = uv + (int64_t)(row >> 1) * s.uv_row + c;
    const int ny = s.W - c, nc = ((s.W + 1) & ~1) - c;                  // valid bytes from c on
    uint32_t yw = 0, cw = 0;
    if (s.words && ny >= 4) {
        yw = *reinterpret_cast<const uint32_t *>(yr);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < ny) yw |= (uint32_t)yr[k] << (8 * k);
    }
    if (s.words && nc >= 4) {
        cw = *reinterpret_cast<const uint32_t *>(cr);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < nc) cw |= (uint32_t)cr[k] << (8 * k);
    }
    uint32_t v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t pair = cw >> (16 * (k >> 1));
        v[k] = k < ny ? nv_rgb(s.k, (yw >> (8 * k)) & 255u, pair & 255u, (pair >> 8) & 255u) : 0u;
    }
    return make_uint4(v[0], v[1], v[2], v[3]);
}

// 64 quads x 4 rows per workgroup
__global__ __launch_bounds__(256) void nv12_to_rgb_kernel(const Nv12RgbArgs p) {
    const int c = (blockIdx.x * 64 + (threadIdx.x & 63)) * 4, row = blockIdx.y * 4 + (threadIdx.x >> 6), b = blockIdx.z;
    if (c >= p.s.W || row >= p.s.H) return;
    const uint4 v = nv_quad(p.s, p.s.y + (int64_t)b * p.s.y_img, p.s.uv + (int64_t)b * p.s.uv_img, row, c);
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

// N = pixels per thread along x of the vertical pass and the stores: 4 or 1 (frames_tile.h)
template <int N>
__global__ __launch_bounds__(256) void nv12_to_input_kernel(const Nv12InputArgs p) {
    extern __shared__ __align__(16) uint32_t nv_lds[];
    uint32_t *stage = nv_lds;                                           // [max_rows][FR_TW] horizontally resampled pixels
    int32_t *wts = reinterpret_cast<int32_t *>(nv_lds + p.o.max_rows * FR_TW);   // [ksx][FR_TW] horizontal weights, tap-major
    uint32_t *raw = nv_lds + (p.o.max_rows + p.o.ksx) * FR_TW;          // [NV_ROWS][max_cols] converted source pixels
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
        const unsigned char *ysrc = p.s.y + (int64_t)b * p.s.y_img, *uvsrc = p.s.uv + (int64_t)b * p.s.uv_img;
        const int nq = p.max_cols >> 2;
        for (int rb = 0; rb < win.nrows; rb += NV_ROWS) {
            const int nr = min(NV_ROWS, win.nrows - rb);
            if (rb) __syncthreads();                                    // the previous step's taps have been read
            for (int r = wv; r < nr; r += 256 / FR_TW)                  // a wave converts a row of the window
                for (int q = col; q < nq; q += FR_TW)
                    *reinterpret_cast<uint4 *>(raw + r * p.max_cols + 4 * q) = nv_quad(p.s, ysrc, uvsrc, win.r0 + rb + r, c0 + 4 * q);
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

// The checks both entry points share; fills `s`
int nv12_source(Nv12Src &s, const unsigned char *y, int64_t y_img, int64_t y_row, const unsigned char *uv, int64_t uv_img,
                int64_t uv_row, int B, int H, int W, int matrix, int full_range) {
    if (!y || !uv || B <= 0 || H <= 0 || W <= 0) return MYDET_E_BADARG;
    if (y_row < W || uv_row < 2 * (((int64_t)W + 1) / 2) || y_img < 0 || uv_img < 0) return MYDET_E_BADARG;
    if (matrix < 0 || matrix > 1 || full_range < 0 || full_range > 1) return MYDET_E_BADARG;
    s.y = y; s.uv = uv; s.y_img = y_img; s.y_row = y_row; s.uv_img = uv_img; s.uv_row = uv_row; s.H = H; s.W = W;
    s.words = (((uintptr_t)y | (uintptr_t)uv | (uintptr_t)y_img | (uintptr_t)y_row | (uintptr_t)uv_img | (uintptr_t)uv_row) & 3) == 0;
    s.k = NV_COEF[matrix][full_range];
    return 0;
}

}  // namespace

extern "C" int mydet_nv12_to_rgb_u8(const unsigned char *y, int64_t y_img_bytes, int64_t y_row_bytes, const unsigned char *uv,
                                    int64_t uv_img_bytes, int64_t uv_row_bytes, int B, int H, int W, unsigned char *dst,
                                    int64_t dst_img_bytes, int64_t dst_row_bytes, int matrix, int full_range, void *stream) {
    Nv12RgbArgs p;
    const int code = nv12_source(p.s, y, y_img_bytes, y_row_bytes, uv, uv_img_bytes, uv_row_bytes, B, H, W, matrix, full_range);
    if (code) return code;
    if (!dst || dst_row_bytes < (int64_t)W * 3 || dst_img_bytes < 0) return MYDET_E_BADARG;
    const int gy = (H + 3) / 4;
    if (B > 65535 || gy > 65535) return MYDET_E_UNSUPP;
    p.dst = dst; p.dst_img = dst_img_bytes; p.dst_row = dst_row_bytes;
    p.dst_words = (((uintptr_t)dst | (uintptr_t)dst_img_bytes | (uintptr_t)dst_row_bytes) & 3) == 0;
    const dim3 grid((unsigned)((W + 255) / 256), (unsigned)gy, (unsigned)B);
    hipLaunchKernelGGL(nv12_to_rgb_kernel, grid, dim3(256), 0, (hipStream_t)stream, p);
    return mydet_launch_status();
}

extern "C" int mydet_nv12_to_input_f32(const unsigned char *y, int64_t y_img_bytes, int64_t y_row_bytes, const unsigned char *uv,
                                       int64_t uv_img_bytes, int64_t uv_row_bytes, int B, int H, int W, int matrix, int full_range,
                                       float *out, int Hp, int Wp, int oh, int ow, int top, int left, const int32_t *bounds_x,
                                       const int32_t *kx, int ksx, const int32_t *bounds_y, const int32_t *ky, int ksy, int norm,
                                       const float *mean3, const float *std3, void *stream) {
    Nv12InputArgs p;
    const int code = nv12_source(p.s, y, y_img_bytes, y_row_bytes, uv, uv_img_bytes, uv_row_bytes, B, H, W, matrix, full_range);
    if (code) return code;
    dim3 grid;
    const int tile = fr_tile_setup(p.o, grid, B, H, W, out, Hp, Wp, oh, ow, top, left, bounds_x, kx, ksx, bounds_y, ky, ksy, norm,
                                   mean3, std3);
    if (tile) return tile;
    // source columns under FR_TW output columns, by the rule of max_rows (frames_tile.h): <= (FR_TW - 1) * scale + ksx, + 2 spare.
    // The column window starts on a quad (+ 3) and is a whole number of quads.
    int64_t cols = FR_TW;
    if (bounds_x) cols = (int64_t)((double)(FR_TW - 1) * (double)W / (double)ow) + ksx + 2;
    cols = (cols + 3 + 3) / 4 * 4;
    if (cols > ((int64_t)W + 3) / 4 * 4) cols = ((int64_t)W + 3) / 4 * 4;
    p.max_cols = (int)cols;
    const size_t lds = fr_tile_lds_bytes(p.o) + (size_t)NV_ROWS * p.max_cols * sizeof(uint32_t);
    if (lds > 64 * 1024) return MYDET_E_UNSUPP;
    if (fr_quad_stores(p.o))
        hipLaunchKernelGGL(nv12_to_input_kernel<4>, grid, dim3(256), lds, (hipStream_t)stream, p);
    else
        hipLaunchKernelGGL(nv12_to_input_kernel<1>, grid, dim3(256), lds, (hipStream_t)stream, p);
    return mydet_launch_status();
}
