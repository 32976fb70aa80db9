// Video frames -> network input in one launch: B uint8 HWC frames of ONE size -> float32 [B,3,Hp,Wp].
//
//   Pillow's bilinear resize to oh x ow (the two-pass 8-bit fixed-point filter of boxops.hip: horizontal pass rounded to
//   uint8, vertical pass on those uint8 values), placed at (top, left) of a zero image of Hp x Wp, then x / 255 and, with
//   norm, (x - mean[c]) / std[c] in the operation order of preprocess_kernel (boxops.hip) -- the floats are the ones
//   mydet_resize_bilinear_u8 + mydet_preprocess_u8_f32 produce, bit for bit, without the uint8 image in between.
//
// A workgroup of 256 threads owns FR_TH x FR_TW output pixels (all three planes).  The vertical taps of its rows span the
// source rows [r0, r1); the horizontally resampled pixels of those rows and the tile's columns go to LDS as one packed
// dword each (r | g << 8 | b << 16, zero outside the window), so every horizontal result is computed once per tile and
// not once per vertical tap.  The vertical pass reads four pixels of a tap row with one 16-byte LDS read; a wave then
// stores whole 256-byte row segments of a plane (16 bytes per lane when Wp % 4 == 0).
//
// LDS: (rows + ksx) * FR_TW dwords, rows <= (FR_TH - 1) * H / oh + ksy + 2.  With MYDET_FRAMES_MAX_TAPS = 17 (a downscale
// of up to 8x: ksize = 2 * ceil(scale) + 1) that is at most 139 + 17 rows of 256 bytes = 39 KiB, and 53 + 7 rows (15 KiB)
// for 1080p -> 360 rows: several workgroups per CU, no opt-in.  Every table entry is clamped before it addresses
// anything, so a malformed table gives wrong pixels, never an access outside the frame or the stage.
#include "common.h"

namespace {

constexpr int FR_TH = 16, FR_TW = 64;

struct FramesArgs {
    const unsigned char *src;
    float *out;
    int64_t src_img, src_row;                  // bytes between frames / rows
    int H, W, Hp, Wp, oh, ow, top, left, ksx, ksy, max_rows, norm;
    const int32_t *bx, *kx, *by, *ky;          // bounds [o][2] = (first tap, taps), weights [o][ks]; null = pass skipped
    float m[3], s[3];
};

__device__ __forceinline__ int fr_clip8(int v) {
    v >>= 22;
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

__device__ __forceinline__ int fr_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// N = pixels per thread along x of the vertical pass and the stores: 4 (float4 stores, Wp % 4 == 0) or 1
template <int N>
__global__ __launch_bounds__(256) void frames_to_input_kernel(const FramesArgs p) {
    extern __shared__ __align__(16) uint32_t fr_lds[];
    uint32_t *stage = fr_lds;                                           // [max_rows][FR_TW] packed pixels
    int32_t *wts = reinterpret_cast<int32_t *>(fr_lds + p.max_rows * FR_TW);   // [ksx][FR_TW] horizontal weights, tap-major
    const int tid = threadIdx.x;
    const int tx0 = blockIdx.x * FR_TW, ty0 = blockIdx.y * FR_TH, b = blockIdx.z;
    const unsigned char *src = p.src + (int64_t)b * p.src_img;

    // rows / columns of the resized image that fall into this tile
    const int wy_lo = max(ty0 - p.top, 0), wy_hi = min(ty0 + FR_TH - p.top, p.oh);
    const int wx_lo = max(tx0 - p.left, 0), wx_hi = min(tx0 + FR_TW - p.left, p.ow);
    const bool live = wy_lo < wy_hi && wx_lo < wx_hi;                   // uniform over the workgroup
    int r0 = 0, nrows = 1;
    if (live) {
        int r1;
        if (p.by) {
            r0 = p.by[2 * wy_lo];
            r1 = p.by[2 * (wy_hi - 1)] + p.by[2 * (wy_hi - 1) + 1];
        } else {
            r0 = wy_lo;
            r1 = wy_hi;
        }
        r0 = fr_clamp(r0, 0, p.H - 1);
        nrows = fr_clamp(r1 - r0, 1, min(p.max_rows, p.H - r0));

        if (p.bx) {
            for (int i = tid; i < FR_TW * p.ksx; i += 256) {
                const int col = i / p.ksx, t = i - col * p.ksx;
                const int wx = tx0 + col - p.left;
                wts[t * FR_TW + col] = (wx >= 0 && wx < p.ow) ? p.kx[wx * p.ksx + t] : 0;
            }
            __syncthreads();
        }
        // horizontal pass: a thread owns one column of the tile and every fourth source row
        const int col = tid & (FR_TW - 1);
        const int wx = tx0 + col - p.left;
        const bool inside = wx >= 0 && wx < p.ow;
        int x0 = 0, nx = 1;
        if (inside) {
            if (p.bx) {
                x0 = fr_clamp(p.bx[2 * wx], 0, p.W - 1);
                nx = fr_clamp(p.bx[2 * wx + 1], 0, min(p.ksx, p.W - x0));
            } else {
                x0 = wx;
            }
        }
        for (int r = tid >> 6; r < nrows; r += 256 / FR_TW) {
            uint32_t v = 0;
            if (inside) {
                const unsigned char *px = src + (int64_t)(r0 + r) * p.src_row + x0 * 3;
                if (p.bx) {
                    int a0 = 1 << 21, a1 = 1 << 21, a2 = 1 << 21;
                    for (int t = 0; t < nx; ++t) {
                        const int w = wts[t * FR_TW + col];
                        a0 += px[3 * t] * w; a1 += px[3 * t + 1] * w; a2 += px[3 * t + 2] * w;
                    }
                    v = (uint32_t)fr_clip8(a0) | ((uint32_t)fr_clip8(a1) << 8) | ((uint32_t)fr_clip8(a2) << 16);
                } else {
                    v = (uint32_t)px[0] | ((uint32_t)px[1] << 8) | ((uint32_t)px[2] << 16);
                }
            }
            stage[r * FR_TW + col] = v;
        }
    }
    __syncthreads();

    // vertical pass + float conversion: a thread owns N neighbouring pixels of a row
    constexpr int XT = FR_TW / N;                                       // threads along x
    const int xq = tid % XT;
    const int ox = tx0 + xq * N;
    if (ox >= p.Wp) return;                                             // N == 4: Wp % 4 == 0, a quad is in or out as a whole
    const int64_t plane = (int64_t)p.Hp * p.Wp;
    for (int ly = tid / XT; ly < FR_TH; ly += 256 / XT) {
        const int oy = ty0 + ly;
        if (oy >= p.Hp) break;
        const int wy = oy - p.top;
        uint32_t q[N];
#pragma unroll
        for (int e = 0; e < N; ++e) q[e] = 0;
        if (live && wy >= 0 && wy < p.oh) {
            if (p.by) {
                const int y0 = p.by[2 * wy], ny = fr_clamp(p.by[2 * wy + 1], 0, p.ksy);
                int acc[N][3];
#pragma unroll
                for (int e = 0; e < N; ++e) acc[e][0] = acc[e][1] = acc[e][2] = 1 << 21;
                for (int j = 0; j < ny; ++j) {
                    const int w = p.ky[wy * p.ksy + j];
                    const int rr = fr_clamp(y0 + j - r0, 0, nrows - 1);
                    uint32_t h[N];
                    if constexpr (N == 4) {
                        const uint4 t4 = *reinterpret_cast<const uint4 *>(stage + rr * FR_TW + xq * 4);
                        h[0] = t4.x; h[1] = t4.y; h[2] = t4.z; h[3] = t4.w;
                    } else {
                        h[0] = stage[rr * FR_TW + xq];
                    }
#pragma unroll
                    for (int e = 0; e < N; ++e) {
                        acc[e][0] += (int)(h[e] & 255u) * w;
                        acc[e][1] += (int)((h[e] >> 8) & 255u) * w;
                        acc[e][2] += (int)((h[e] >> 16) & 255u) * w;
                    }
                }
#pragma unroll
                for (int e = 0; e < N; ++e)
                    q[e] = (uint32_t)fr_clip8(acc[e][0]) | ((uint32_t)fr_clip8(acc[e][1]) << 8) | ((uint32_t)fr_clip8(acc[e][2]) << 16);
            } else {
                const int rr = fr_clamp(wy - r0, 0, nrows - 1);
                if constexpr (N == 4) {
                    const uint4 t4 = *reinterpret_cast<const uint4 *>(stage + rr * FR_TW + xq * 4);
                    q[0] = t4.x; q[1] = t4.y; q[2] = t4.z; q[3] = t4.w;
                } else {
                    q[0] = stage[rr * FR_TW + xq];
                }
            }
        }
        float *o = p.out + (int64_t)b * 3 * plane + (int64_t)oy * p.Wp + ox;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float f[N];
#pragma unroll
            for (int e = 0; e < N; ++e) {
                f[e] = (float)((q[e] >> (8 * c)) & 255u) / 255.0f;
                if (p.norm) f[e] = (f[e] - p.m[c]) / p.s[c];
            }
            if constexpr (N == 4) {
                f32x4 v = {f[0], f[1], f[2], f[3]};
                *reinterpret_cast<f32x4 *>(o + c * plane) = v;
            } else {
                o[c * plane] = f[0];
            }
        }
    }
}

}  // namespace

extern "C" int mydet_frames_to_input_f32(const unsigned char *src, int B, int H, int W, int64_t src_img_bytes,
                                         int64_t src_row_bytes, float *out, int Hp, int Wp, int oh, int ow, int top, int left,
                                         const int32_t *bounds_x, const int32_t *kx, int ksx, const int32_t *bounds_y,
                                         const int32_t *ky, int ksy, int norm, const float *mean3, const float *std3,
                                         void *stream) {
    if (!src || !out || B <= 0 || H <= 0 || W <= 0 || Hp <= 0 || Wp <= 0 || oh <= 0 || ow <= 0 || top < 0 || left < 0)
        return MYDET_E_BADARG;
    if (src_row_bytes < (int64_t)W * 3 || src_img_bytes < 0) return MYDET_E_BADARG;
    if ((int64_t)top + oh > Hp || (int64_t)left + ow > Wp) return MYDET_E_BADARG;
    if ((bounds_x == nullptr) != (kx == nullptr) || (bounds_y == nullptr) != (ky == nullptr)) return MYDET_E_BADARG;
    if ((!bounds_x && W != ow) || (!bounds_y && H != oh)) return MYDET_E_BADARG;
    if ((bounds_x && (ksx <= 0 || ksx > MYDET_FRAMES_MAX_TAPS)) || (bounds_y && (ksy <= 0 || ksy > MYDET_FRAMES_MAX_TAPS)))
        return MYDET_E_BADARG;
    if (norm && (!mean3 || !std3)) return MYDET_E_BADARG;
    const int gy = (Hp + FR_TH - 1) / FR_TH;
    if (B > 65535 || gy > 65535) return MYDET_E_UNSUPP;
    FramesArgs p;
    p.src = src; p.out = out; p.src_img = src_img_bytes; p.src_row = src_row_bytes;
    p.H = H; p.W = W; p.Hp = Hp; p.Wp = Wp; p.oh = oh; p.ow = ow; p.top = top; p.left = left;
    p.ksx = bounds_x ? ksx : 0; p.ksy = bounds_y ? ksy : 0; p.norm = norm ? 1 : 0;
    p.bx = bounds_x; p.kx = kx; p.by = bounds_y; p.ky = ky;
    for (int c = 0; c < 3; ++c) {
        p.m[c] = norm ? mean3[c] : 0.f;
        p.s[c] = norm ? std3[c] : 1.f;
    }
    // source rows under FR_TH output rows: last tap of the last row - first tap of the first <= (FR_TH - 1) * scale + 2 * support + 1
    // <= (FR_TH - 1) * scale + ksy by Pillow's rule (support = max(scale, 1), ksize = 2 * ceil(support) + 1); + 2 spare
    int64_t rows = FR_TH;
    if (bounds_y) rows = (int64_t)((double)(FR_TH - 1) * (double)H / (double)oh) + ksy + 2;
    if (rows > H) rows = H;
    p.max_rows = (int)rows;
    const size_t lds = (size_t)(p.max_rows + p.ksx) * FR_TW * sizeof(uint32_t);
    if (lds > 64 * 1024) return MYDET_E_UNSUPP;
    const dim3 grid((unsigned)((Wp + FR_TW - 1) / FR_TW), (unsigned)gy, (unsigned)B);
    if ((Wp & 3) == 0 && ((uintptr_t)out & 15) == 0)
        hipLaunchKernelGGL(frames_to_input_kernel<4>, grid, dim3(256), lds, (hipStream_t)stream, p);
    else
        hipLaunchKernelGGL(frames_to_input_kernel<1>, grid, dim3(256), lds, (hipStream_t)stream, p);
    return mydet_launch_status();
}
