// The tile frame of the implicit-GEMM convolutions (conv_igemm.hip: conv_igemm_kernel, conv_igemm_b3_kernel, conv_igemm_b3w_kernel and
// conv_fixup_kernel).  Defined here, once: the argument block, the tile origin and the A window, a staged row's address and tap mask,
// the K range of a block and the uniform tap cursor, the accumulators and the lane's scale / shift, the two-buffer K loop, and the end
// of a tile (raw partial tile for the fixup, or the fused epilogue).  What a kernel keeps is its own staging layout (LDS row format,
// weight path, GATE / CAT operand) and its compute lambda; the wide form also keeps its ring loop.
#pragma once
#include "common.h"

namespace {

constexpr unsigned OOB = 0xFFFFFFFFu;

struct ConvArgs {
    const float *x, *w, *scale, *shift, *res, *gate;
    float *y;
    int64_t ldx, ldr, ldy;
    int B, H, W, Cin, Cout, KH, KW, stride, pad_t, pad_l, Ho, Wo, act;
    int M, K, ntiles, nblk;
    int tile0, splits;        // split-K tail: first logical tile of this launch, K slices per tile (1 = whole K)
    float *ws;                // split-K partial accumulators
    size_t ws_bytes;
    // CAT (1x1 only): channels [0, C1) of A come from x1 = a [B, H/2, W/2, ldx1] map read through nearest 2x upsampling, the
    // remaining Cin - C1 from x -- conv1x1(cat((up2x(x1), x), 1)) without the concatenated tensor
    const float *x1;
    int64_t ldx1;
    int C1;
    // split-bf16 form (conv_igemm_b3_kernel): the weights as three bfloat16 planes [3][Cout][K] with w = p0 + p1 + p2
    const unsigned short *wsplit;
};

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ f32x4 buf_load16(__amdgpu_buffer_rsrc_t rsrc, unsigned voff) {
    return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc, voff, 0, 0));
}

// Epilogue: lane = output channel, register = output pixel.  Stores (and residual loads) are
// buffer ops whose per-lane offset is fixed and whose row term is a scalar: one v_add per element.
// Ragged tiles route out-of-range elements to offset 0xFFFFFFFF, which the range check drops.
template <int ACT, bool RES, bool FULL, int TM, int TN>
__device__ __forceinline__ void epilogue(const ConvArgs &p, f32x16 (&acc)[TM][TN], int m_base, int n_base,
                                         int fr, int fh, const float (&pscl)[TN], const float (&psft)[TN]) {
    const __amdgpu_buffer_rsrc_t yr = mydet_rsrc(p.y, (int64_t)p.M * p.ldy * 4);
    const __amdgpu_buffer_rsrc_t rr = mydet_rsrc(RES ? p.res : p.y, (int64_t)p.M * (RES ? p.ldr : p.ldy) * 4);
    const unsigned ldy4 = (unsigned)p.ldy * 4u, ldr4 = (unsigned)p.ldr * 4u;
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int n = n_base + j * 32 + fr;
        const bool nok = FULL || n < p.Cout;
        const float scl = pscl[j], sft = psft[j];      // requested before the K loop (a round trip per workgroup otherwise)
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            const int mrow = m_base + i * 32 + 4 * fh;          // + (r&3) + 8*(r>>2)
            const unsigned ybase = (unsigned)mrow * ldy4 + (unsigned)n * 4u;
            const unsigned rbase = (unsigned)mrow * ldr4 + (unsigned)n * 4u;
            float rv[16];
            if (RES) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int dr = (r & 3) + 8 * (r >> 2);
                    const bool ok = FULL || (nok && mrow + dr < p.M);
                    rv[r] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(
                                                          rr, ok ? rbase + (unsigned)dr * ldr4 : OOB, 0, 0));
                }
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int dr = (r & 3) + 8 * (r >> 2);
                float v = acc[i][j][r] * scl + sft;
                if (ACT == MYDET_ACT_LEAKY) v = v > 0.0f ? v : v * 0.1f;
                if (ACT == MYDET_ACT_SWISH) v = v * mydet_sigmoid_fast(v);
                if (RES) v += rv[r];
                const bool ok = FULL || (nok && mrow + dr < p.M);
                __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), yr,
                                                      ok ? ybase + (unsigned)dr * ldy4 : OOB, 0, 0);
            }
        }
    }
}

// ---- tile origin and A window.  SPLIT: block = (tail tile, K slice); otherwise one block per tile, XCD-grouped.  The window of the
// A descriptor starts at the image holding the tile's first row.
struct IgTile {
    int m0, n0, hwo, b0;
    __amdgpu_buffer_rsrc_t xr;
};
template <bool SPLIT, int BM, int BN>
__device__ __forceinline__ IgTile ig_tile(const ConvArgs &p) {
    IgTile t;
    const int lid = SPLIT ? p.tile0 + (int)blockIdx.x / p.splits : mydet_xcd_remap(blockIdx.x, p.nblk);
    t.m0 = (lid / p.ntiles) * BM;
    t.n0 = (lid % p.ntiles) * BN;
    t.hwo = p.Ho * p.Wo;
    t.b0 = t.m0 / t.hwo;
    const int64_t img = (int64_t)p.H * p.W * p.ldx;
    t.xr = mydet_rsrc(p.x + t.b0 * img, (p.B - t.b0) * img * 4);
    return t;
}

// ---- one staged row of A: output pixel m, this thread's channel quad sc.  aoff: byte offset of tap (0,0), channel 4*sc, from the
// window base; amask bit t: tap t of the row is inside the image (0 for rows past M); b: the row's image (for the gate), (oh, ow)
// its output pixel (general path only: the CAT operand).
// flat = pointwise, stride 1, unpadded (uniform): input pixel == output pixel, no index arithmetic beyond the row number (the
// three divisions per row of the general path are pure latency in a small-grid launch)
__device__ __forceinline__ bool ig_flat(const ConvArgs &p) {
    return p.KH * p.KW == 1 && p.stride == 1 && p.pad_t == 0 && p.pad_l == 0 && p.Ho == p.H && p.Wo == p.W;
}
struct IgRow {
    int aoff;
    unsigned amask;
    int b, oh, ow;
};
__device__ __forceinline__ IgRow ig_row(const ConvArgs &p, const IgTile &t, bool flat, int m, int sc) {
    IgRow r;
    const int mm = m < p.M ? m : p.M - 1;
    if (flat) {
        r.aoff = (int)(((int64_t)(mm - t.b0 * t.hwo) * p.ldx + sc * 4) * 4);
        r.amask = m < p.M ? 1u : 0u;
        r.b = mm / t.hwo;
        r.oh = r.ow = 0;
        return r;
    }
    const int ntaps = p.KH * p.KW;
    const int ow = mm % p.Wo, q = mm / p.Wo;
    const int oh = q % p.Ho, b = q / p.Ho;
    const int ih0 = oh * p.stride - p.pad_t, iw0 = ow * p.stride - p.pad_l;
    r.aoff = (int)((((int64_t)(b - t.b0) * p.H + ih0) * p.W + iw0) * p.ldx + sc * 4) * 4;
    unsigned mask = 0;
    for (int tp = 0; tp < ntaps; ++tp) {
        const int kh = tp / p.KW, kw = tp - kh * p.KW;
        if ((unsigned)(ih0 + kh) < (unsigned)p.H && (unsigned)(iw0 + kw) < (unsigned)p.W) mask |= 1u << tp;
    }
    r.amask = m < p.M ? mask : 0u;
    r.b = b; r.oh = oh; r.ow = ow;
    return r;
}

// ---- K range of a block, in slabs: [kt0, nk) of the layer's nk_all (SPLIT: this block's slice)
template <bool SPLIT>
__device__ __forceinline__ void ig_k_range(const ConvArgs &p, int nk_all, int &kt0, int &nk) {
    kt0 = 0; nk = nk_all;
    if (SPLIT) {
        const int sp = (int)blockIdx.x % p.splits;
        kt0 = (int)((unsigned)(nk_all * sp) / (unsigned)p.splits);          // (nk_all * splits < 2^31: no 64-bit division)
        nk = (int)((unsigned)(nk_all * (sp + 1)) / (unsigned)p.splits);
    }
}

// ---- uniform tap cursor of the slab being requested (a slab never straddles taps): tap, its first channel, the tap's byte offset
struct IgTapCursor {
    int tap = 0, c0 = 0, tapoff = 0;
    __device__ __forceinline__ void set_tap(const ConvArgs &p, int t) {
        tap = t;
        const int kh = tap / p.KW, kw = tap - kh * p.KW;
        tapoff = (int)(((int64_t)kh * p.W + kw) * p.ldx) * 4;
    }
    __device__ __forceinline__ void seek(const ConvArgs &p, int k0) {       // SPLIT: a slice starts inside K
        set_tap(p, k0 / p.Cin);
        c0 = k0 - tap * p.Cin;
    }
    __device__ __forceinline__ void advance(const ConvArgs &p, int BK) {
        c0 += BK;
        if (c0 == p.Cin) {                            // uniform: next tap
            c0 = 0;
            set_tap(p, tap + 1);
        }
    }
};

// ---- accumulators, and this lane's output channels' scale / shift (requested before the K loop: in flight under it)
template <int TM, int TN>
__device__ __forceinline__ void ig_zero(f32x16 (&acc)[TM][TN]) {
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
}
template <bool SPLIT, int TN>
__device__ __forceinline__ void ig_scale_shift(const ConvArgs &p, int n_base, int fr, float (&pscl)[TN], float (&psft)[TN]) {
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int n = n_base + j * 32 + fr;
        const int nc = n < p.Cout ? n : 0;
        pscl[j] = (!SPLIT && p.scale) ? p.scale[nc] : 1.0f;
        psft[j] = (!SPLIT && p.shift) ? p.shift[nc] : 0.0f;
    }
}

// ---- K loop of the double-buffered kernels.  LDS holds two slabs (the one being multiplied, the next one), registers PF more: the
// loads of slabs kt+2 .. kt+1+PF are in flight while slab kt is multiplied, so a workgroup alone on its CU (small grids: batch-1
// layers, the MBConv 1x1 convs of one batch lane) has two MFMA phases to cover a load round trip instead of one -- with one slab
// in flight those loops ran at the L2 latency (0.67 us per slab against 0.43 us of MFMA work).
// Prefetches past the last slab are unconditional: load_slab masks them off or keeps them in range -- harmless, never consumed.
// RA / RB: one register set of the A / B operand (array types); load_slab(kt, a, b), store_slab(buf, a, b), compute(buf).
template <int PF, class RA, class RB, class Load, class Store, class Compute>
__device__ __forceinline__ void ig_k_loop(int kt0, int nk, Load &&load_slab, Store &&store_slab, Compute &&compute) {
    RA areg[PF];
    RB breg[PF];
    load_slab(kt0, areg[0], breg[0]);
    store_slab(0, areg[0], breg[0]);
#pragma unroll
    for (int d = 0; d < PF; ++d) load_slab(kt0 + 1 + d, areg[d], breg[d]);
    __syncthreads();
    int buf = 0;
    for (int kt = kt0; kt < nk; kt += PF) {
#pragma unroll
        for (int d = 0; d < PF; ++d) {               // register set d holds slab kt + d + 1
            if (kt + d >= nk) break;
            compute(buf);
            store_slab(buf ^ 1, areg[d], breg[d]);
            load_slab(kt + d + 1 + PF, areg[d], breg[d]);
            __syncthreads();
            buf ^= 1;
        }
    }
}

// ---- end of a tile.  SPLIT: the raw partial tile, [vec4][thread] so lanes store contiguously; summed by conv_fixup_kernel.
// Otherwise the fused epilogue, FULL or ragged.
template <int ACT, bool RES, bool SPLIT, int BM, int BN, int NT, int TM, int TN>
__device__ __forceinline__ void ig_finish(const ConvArgs &p, f32x16 (&acc)[TM][TN], int m0, int n0, int m_base, int n_base, int tid,
                                          int fr, int fh, const float (&pscl)[TN], const float (&psft)[TN]) {
    if (SPLIT) {
        constexpr int NV4 = TM * TN * 4;
        f32x4 *dst = reinterpret_cast<f32x4 *>(p.ws) + (int64_t)blockIdx.x * NV4 * NT + tid;
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int v = 0; v < 4; ++v)
                    dst[((i * TN + j) * 4 + v) * NT] =
                        f32x4{acc[i][j][4 * v], acc[i][j][4 * v + 1], acc[i][j][4 * v + 2], acc[i][j][4 * v + 3]};
        return;
    }
    if ((m0 + BM <= p.M) && (n0 + BN <= p.Cout))
        epilogue<ACT, RES, true, TM, TN>(p, acc, m_base, n_base, fr, fh, pscl, psft);
    else
        epilogue<ACT, RES, false, TM, TN>(p, acc, m_base, n_base, fr, fh, pscl, psft);
}

}  // namespace
