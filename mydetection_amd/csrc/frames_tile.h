// The tile pipeline of the frame-input kernels (frames.hip: uint8 RGB frames, yuv420.hip: 4:2:0 planes in any layout): both
// give float32 [B,3,Hp,Wp] and differ only in where the horizontal taps come from.
//
// A workgroup of 256 threads owns FR_TH x FR_TW output pixels (all three planes).  The vertical taps of its rows span the
// source rows [r0, r0 + nrows); the horizontally resampled pixels of those rows and the tile's columns go to the LDS stage
// as one packed dword each (zero outside the window), so every horizontal result is computed once per tile and not once per
// vertical tap.  The kernel fills the stage (fr_window, fr_stage_weights, fr_column and its own tap loads), then
// fr_vertical_store reads four pixels of a tap row with one 16-byte LDS read and a wave stores whole 256-byte row segments
// of a plane (16 bytes per lane when Wp % 4 == 0).
//
// LDS: [max_rows][FR_TW] stage, then [ksx][FR_TW] horizontal weights (fr_tile_lds_bytes), then whatever the kernel adds.
// Every table entry is clamped before it addresses anything, so a malformed table gives wrong pixels, never an access
// outside the source or the stage.
#pragma once
#include "pixel_math.h"

namespace {

constexpr int FR_TH = 16, FR_TW = 64;

// The output side of a launch, by value in the kernel's arguments
struct FrOut {
    float *out;
    int Hp, Wp, oh, ow, top, left, ksx, ksy, max_rows, norm;
    const int32_t *bx, *kx, *by, *ky;          // bounds [o][2] = (first tap, taps), weights [o][ks]; null = pass skipped
    float m[3], s[3];
};

// What a tile needs of the source: uniform over the workgroup
struct FrWindow {
    bool live;                                 // the tile holds pixels of the resized image
    int wx_lo;                                 // its first column of the resized image
    int r0, nrows;                             // source rows [r0, r0 + nrows) feed its vertical taps
};

__device__ __forceinline__ FrWindow fr_window(const FrOut &p, int H, int tx0, int ty0) {
    const int wy_lo = max(ty0 - p.top, 0), wy_hi = min(ty0 + FR_TH - p.top, p.oh);
    const int wx_lo = max(tx0 - p.left, 0), wx_hi = min(tx0 + FR_TW - p.left, p.ow);
    FrWindow w = {wy_lo < wy_hi && wx_lo < wx_hi, wx_lo, 0, 1};
    if (w.live) {
        int r1;
        if (p.by) {
            w.r0 = p.by[2 * wy_lo];
            r1 = p.by[2 * (wy_hi - 1)] + p.by[2 * (wy_hi - 1) + 1];
        } else {
            w.r0 = wy_lo;
            r1 = wy_hi;
        }
        w.r0 = px_clamp(w.r0, 0, H - 1);
        w.nrows = px_clamp(r1 - w.r0, 1, min(p.max_rows, H - w.r0));
    }
    return w;
}

// wts[ksx][FR_TW]: the horizontal weights of the tile's columns, tap-major, zero outside the window.  No barrier here.
__device__ __forceinline__ void fr_stage_weights(const FrOut &p, int32_t *wts, int tx0, int tid) {
    for (int i = tid; i < FR_TW * p.ksx; i += 256) {
        const int col = i / p.ksx, t = i - col * p.ksx;
        const int wx = tx0 + col - p.left;
        wts[t * FR_TW + col] = (wx >= 0 && wx < p.ow) ? p.kx[wx * p.ksx + t] : 0;
    }
}

// The taps of tile column `col`: source columns [x0, x0 + nx) when it is inside the window
struct FrColumn {
    bool inside;
    int x0, nx;
};

__device__ __forceinline__ FrColumn fr_column(const FrOut &p, int W, int tx0, int col) {
    const int wx = tx0 + col - p.left;
    FrColumn c = {wx >= 0 && wx < p.ow, 0, 1};
    if (c.inside) {
        if (p.bx) {
            c.x0 = px_clamp(p.bx[2 * wx], 0, W - 1);
            c.nx = px_clamp(p.bx[2 * wx + 1], 0, min(p.ksx, W - c.x0));
        } else {
            c.x0 = wx;
        }
    }
    return c;
}

// Mirrored views (MYDET_VIEW_HFLIP / MYDET_VIEW_VFLIP, the *_flip_f32 entry points): the window, the tables and the stage are
// those of the mirrored frame, and only the address of a tap changes -- row y of the mirrored frame is row H-1-y of the
// frame in memory, column x is column W-1-x.  fr_window / fr_column give mirrored coordinates; the kernels pass every row
// and column they read through these two.  FLIP = false instances never call them with a non-zero `flip`.
__device__ __forceinline__ int fr_src_row(int flip, int H, int y) { return (flip & MYDET_VIEW_VFLIP) ? H - 1 - y : y; }
__device__ __forceinline__ int fr_src_col(int flip, int W, int x) { return (flip & MYDET_VIEW_HFLIP) ? W - 1 - x : x; }

inline int fr_flip_arg(int flip) { return (flip & ~(MYDET_VIEW_HFLIP | MYDET_VIEW_VFLIP)) ? MYDET_E_BADARG : 0; }

template <int N>
__device__ __forceinline__ void fr_stage_read(const uint32_t *stage, int rr, int xq, uint32_t (&h)[N]) {
    if constexpr (N == 4) {
        const uint4 t4 = *reinterpret_cast<const uint4 *>(stage + rr * FR_TW + xq * 4);
        h[0] = t4.x; h[1] = t4.y; h[2] = t4.z; h[3] = t4.w;
    } else {
        h[0] = stage[rr * FR_TW + xq];
    }
}

// Vertical pass + float conversion + stores, after the barrier that completes the stage.  A thread owns N neighbouring
// pixels of a row: N = 4 (float4 stores, Wp % 4 == 0 and `out` 16-byte aligned) or 1.
template <int N>
__device__ __forceinline__ void fr_vertical_store(const FrOut &p, const uint32_t *stage, const FrWindow &win, int tx0, int ty0,
                                                  int b, int tid) {
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
        if (win.live && wy >= 0 && wy < p.oh) {
            if (p.by) {
                const int y0 = p.by[2 * wy], ny = px_clamp(p.by[2 * wy + 1], 0, p.ksy);
                PxFilter acc[N];
                for (int j = 0; j < ny; ++j) {
                    const int w = p.ky[wy * p.ksy + j];
                    uint32_t h[N];
                    fr_stage_read<N>(stage, px_clamp(y0 + j - win.r0, 0, win.nrows - 1), xq, h);
#pragma unroll
                    for (int e = 0; e < N; ++e) acc[e].add(h[e], w);
                }
#pragma unroll
                for (int e = 0; e < N; ++e) q[e] = acc[e].pixel();
            } else {
                fr_stage_read<N>(stage, px_clamp(wy - win.r0, 0, win.nrows - 1), xq, q);
            }
        }
        float *o = p.out + (int64_t)b * 3 * plane + (int64_t)oy * p.Wp + ox;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float f[N];
#pragma unroll
            for (int e = 0; e < N; ++e) f[e] = px_to_float(px_chan(q[e], c), p.norm, p.m[c], p.s[c]);
            if constexpr (N == 4) {
                f32x4 v = {f[0], f[1], f[2], f[3]};
                *reinterpret_cast<f32x4 *>(o + c * plane) = v;
            } else {
                o[c * plane] = f[0];
            }
        }
    }
}

// Host side of a launch: the checks on the output arguments, `p`, and the grid.  0, MYDET_E_BADARG or MYDET_E_UNSUPP.
inline int fr_tile_setup(FrOut &p, dim3 &grid, int B, int H, int W, float *out, int Hp, int Wp, int oh, int ow, int top, int left,
                         const int32_t *bounds_x, const int32_t *kx, int ksx, const int32_t *bounds_y, const int32_t *ky, int ksy,
                         int norm, const float *mean3, const float *std3) {
    if (!out || Hp <= 0 || Wp <= 0 || oh <= 0 || ow <= 0 || top < 0 || left < 0) return MYDET_E_BADARG;
    if ((int64_t)top + oh > Hp || (int64_t)left + ow > Wp) return MYDET_E_BADARG;
    if ((bounds_x == nullptr) != (kx == nullptr) || (bounds_y == nullptr) != (ky == nullptr)) return MYDET_E_BADARG;
    if ((!bounds_x && W != ow) || (!bounds_y && H != oh)) return MYDET_E_BADARG;
    if ((bounds_x && (ksx <= 0 || ksx > MYDET_FRAMES_MAX_TAPS)) || (bounds_y && (ksy <= 0 || ksy > MYDET_FRAMES_MAX_TAPS)))
        return MYDET_E_BADARG;
    if (norm && (!mean3 || !std3)) return MYDET_E_BADARG;
    const int gy = (Hp + FR_TH - 1) / FR_TH;
    if (B > 65535 || gy > 65535) return MYDET_E_UNSUPP;
    p.out = out; p.Hp = Hp; p.Wp = Wp; p.oh = oh; p.ow = ow; p.top = top; p.left = left;
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
    grid = dim3((unsigned)((Wp + FR_TW - 1) / FR_TW), (unsigned)gy, (unsigned)B);
    return 0;
}

// Bytes of the stage and the horizontal weights; a kernel's own LDS follows them
inline size_t fr_tile_lds_bytes(const FrOut &p) { return (size_t)(p.max_rows + p.ksx) * FR_TW * sizeof(uint32_t); }

// The N = 4 form of a kernel can be launched
inline bool fr_quad_stores(const FrOut &p) { return (p.Wp & 3) == 0 && ((uintptr_t)p.out & 15) == 0; }

}  // namespace
