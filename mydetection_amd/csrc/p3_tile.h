// The tile of the patch-resident 3x3 kernels (conv_p3.hip: the patch comes from global memory; conv_stem_p3.hip: the workgroup computes
// it): a workgroup of 4 waves owns 128 output pixels x BN output channels and reads the MFMA A fragments of the nine taps straight out
// of ONE 16-channel slab of its input patch, resident in LDS as three bf16 planes.  Defined here, once: the patch geometry and layout,
// the store of a channel quad into the planes, the lane roles and weight-fragment addresses of the main phase, and the epilogue.  The
// nine-tap loop itself (load_b / compute lambdas, three B fragments in flight) is still written out in each kernel: moved into
// this header as members or as returned lambdas it compiled to a different register allocation (stride 1, BN 128: 174 instead of
// 248 VGPRs, the A-fragment reads that neighbouring row blocks share no longer merged), so it stays where its code is unchanged.
// How the patch of the next slab gets into LDS, and the barriers around that, is the including kernel's business.
//
// Patch layout (one plane; 32 bytes = 16 bf16 per position, the two 16-byte halves swapped where sigma = 1):
//   stride 2: position = py * ROWLEN + (px & 1) * PJ0 + (px >> 1)   (columns split by parity: the 16 pixels an MFMA row block reads
//             for one tap are consecutive positions)
//   stride 1: position = py * ROWLEN + px
//   found by exhaustive search (tools/r06/p3_layout_search.py) over (row length, swizzle) against the ds_read_b128 lane groups of
//   MI355X_MICROARCH.md: every fragment read of every tap touches sixteen distinct 16-byte bank slots per lane group (conflict-free);
//   the staging writes of 4 consecutive positions are 128 contiguous bytes.
// Weights: pre-split planes (mydet_split_bf16_f32, slab kt = tap * Cin/16 + slab) that never touch LDS: a wave owns 32 output channels
// and its MFMA B fragment of a (slab, tap, plane) is ONE coalesced 1 KB load -- the planes store each 32-row block as the 64 16-byte
// units of exactly that fragment -- requested three taps ahead.
#pragma once
#include "common.h"
#include "split_bf16.h"

// conv_p3.hip: the tile plan of an Ho x Wo x Cout output map (host only).  strip: shape of the tiles over the remainder columns behind
// the tx_n * 16 whole ones (0: none, the last 8 x 16 column is ragged); strips = false: never.  Library-internal.
struct P3Plan {
    int BN, strip, tx_n, ty_n, main_tiles, tiles_img, ntn, lds;       // lds: dynamic LDS bytes of the kernel form
};
P3Plan mydet_p3_plan(int Ho, int Wo, int Cout, int stride, bool strips);

namespace {

constexpr unsigned P3_OOB = 0xFFFFFFFFu;
constexpr int P3_COUT_PAD = 256;                 // rows of the weight planes (split_bf16_kernel)
constexpr int P3_ROWB = 32;                      // bytes of a patch position in one plane

// Tile shapes.  SHAPE 0: 8 rows x 16 columns of output pixels (both strides).  SHAPE 1 / 2 (stride 2): 16 x 8 and 32 x 4 STRIP tiles for
// the remainder columns of a map whose width is 16 n + 8 / 16 n + 4 (Darknet-53 at 640^2: the 40- and 20-pixel maps), run by the
// last workgroups of the same launch.  TWL = log2(tile width); PH = patch rows; ROWLEN = positions per patch row; PJ0 = positions
// of the even columns (stride 2: the odd columns follow them).  sigma (the 16-byte half swap of a position) = bit 3 of the column
// index j, plus bit 1 of the patch row for the strip shapes: each found conflict-free by tools/r06/p3_layout_search.py.
template <int S, int SHAPE> struct P3Shape;
template <> struct P3Shape<2, 0> { static constexpr int TH = 8, TWL = 4, PH = 17, ROWLEN = 36, PJ0 = 17; };
template <> struct P3Shape<1, 0> { static constexpr int TH = 8, TWL = 4, PH = 10, ROWLEN = 24, PJ0 = 0; };
template <> struct P3Shape<2, 1> { static constexpr int TH = 16, TWL = 3, PH = 33, ROWLEN = 20, PJ0 = 9; };
template <> struct P3Shape<2, 2> { static constexpr int TH = 32, TWL = 2, PH = 65, ROWLEN = 9, PJ0 = 5; };
template <int S, int SHAPE> struct P3Geom : P3Shape<S, SHAPE> {
    typedef P3Shape<S, SHAPE> G;
    static constexpr int TW = 1 << G::TWL, RPB = 32 / TW;          // RPB: output rows per 32-row MFMA block
    static constexpr int PW = S * (TW - 1) + 3;                    // patch columns
    static constexpr int NPOS = G::PH * G::ROWLEN, PLANE = NPOS * P3_ROWB, LDS = 3 * PLANE;
    static_assert(G::TH * TW == 128 && G::PH == S * (G::TH - 1) + 3 && PW <= (S == 2 ? 2 * G::PJ0 - 1 : G::ROWLEN), "patch geometry");
};
template <int SHAPE> __device__ __forceinline__ int p3_sigma(int py, int j) { return SHAPE == 0 ? (j >> 3) & 1 : ((j >> 3) + (py >> 1)) & 1; }

// Position and half swap of patch pixel (py, px)
template <int S, int SHAPE> __device__ __forceinline__ int p3_pos(int py, int px) {
    typedef P3Geom<S, SHAPE> G;
    return S == 2 ? py * G::ROWLEN + (px & 1) * G::PJ0 + (px >> 1) : py * G::ROWLEN + px;
}
template <int S, int SHAPE> __device__ __forceinline__ int p3_pix_sigma(int py, int px) { return p3_sigma<SHAPE>(py, S == 2 ? px >> 1 : px); }

// Byte offset in a plane of channels 8 half + 4 lo .. + 3 of the slab at position pos (half swap sig), and the store of those four
// channels, cut into their three pieces, into the three planes
__device__ __forceinline__ int p3_quad_off(int pos, int sig, int half, int lo) { return pos * P3_ROWB + ((half ^ sig) * 16) + lo * 8; }
template <int S, int SHAPE> __device__ __forceinline__ void p3_store_quad(char *patch, int off, const f32x4 v) {
    constexpr int PLANE = P3Geom<S, SHAPE>::PLANE;
    bf16x4 q0, q1, q2;
    split3(v, q0, q1, q2);
    char *d = patch + off;
    *reinterpret_cast<bf16x4 *>(d) = q0;
    *reinterpret_cast<bf16x4 *>(d + PLANE) = q1;
    *reinterpret_cast<bf16x4 *>(d + 2 * PLANE) = q2;
}

// The lane's 16-byte unit of a 32-row block in a (slab, plane) piece of the weight planes (split_bf16_kernel)
__device__ __forceinline__ unsigned p3_b_unit(int fr, int fh) { return (unsigned)((2 * fr + (fh ^ ((fr >> 2) & 1))) * 16); }

// One thread's part of a tile of shape SHAPE at stride S x BN output channels (64 | 128): waves = (4 / (BN / 32)) row groups x
// (BN / 32) column blocks of 32; wave (wm, wn): 32 * TM rows x 32 columns.
template <int S, int BN, int SHAPE> struct P3Main {
    typedef P3Geom<S, SHAPE> G;
    static constexpr int TWL = G::TWL, TW = G::TW, RPB = G::RPB, ROWLEN = G::ROWLEN, PLANE = G::PLANE;
    static constexpr int WN = BN / 32, WM = 4 / WN, TM = 4 / WM;

    const int wave, lane, wm, wn, fr, fh;
    int nsl;                                         // 16-channel slabs
    __amdgpu_buffer_rsrc_t wr;
    unsigned boff, plane_bytes, slab_bytes;
    int oxl, nch;                                    // the lane's column of the tile; its output channel
    float pscl, psft;
    // The registers that the (unrolled) loops of the main phase index: the kernel's own, captured by its tap lambdas
    struct Regs {
        int apos[TM], apy[TM];                       // patch position / patch row of the lane's row for tap (0, 0)
        f32x16 acc[TM];
        bf16x8 breg[3][3];                           // B fragments of three (slab, tap) steps in flight
    };

    __device__ __forceinline__ explicit P3Main(int tid)
        : wave(tid >> 6), lane(tid & 63), wm(wave / WN), wn(wave % WN), fr(lane & 31), fh(lane >> 5) {}

    // the weight planes of a layer of nsl_ slabs; n0: first output channel of the workgroup
    __device__ __forceinline__ void weights(const unsigned short *wsplit, int Cout, int nsl_, int n0) {
        const int CoutP = (Cout + P3_COUT_PAD - 1) / P3_COUT_PAD * P3_COUT_PAD;
        nsl = nsl_;
        wr = mydet_rsrc(wsplit, (int64_t)9 * nsl * 3 * CoutP * 32);
        boff = (unsigned)((n0 + wn * 32) * 32) + p3_b_unit(fr, fh);
        plane_bytes = (unsigned)CoutP * 32u;
        slab_bytes = 3u * plane_bytes;
    }

    // the lane's rows of the tile, zero accumulators, the lane's channel and its scale / shift
    __device__ __forceinline__ void rows(Regs &r, const float *scale, const float *shift, int Cout, int n0) {
        oxl = fr & (TW - 1);
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            const int oyl = wm * (TM * RPB) + i * RPB + (fr >> TWL);
            r.apy[i] = S * oyl;
            r.apos[i] = r.apy[i] * ROWLEN + oxl;
        }
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int e = 0; e < 16; ++e) r.acc[i][e] = 0.f;
        nch = n0 + wn * 32 + fr;
        pscl = scale ? scale[nch < Cout ? nch : 0] : 1.0f;
        psft = shift ? shift[nch < Cout ? nch : 0] : 0.0f;
    }

    // Epilogue of the tile at (image b, output row oy0, column ox0) of a [B, Ho, Wo, ldy] map: lane = output channel, register =
    // output pixel of the RPB-row x TW-column block (row r of the block: (r >> TWL, r & (TW - 1))); scale / shift / activation /
    // residual as conv_igemm's.  Pixels and channels outside the map go to offset P3_OOB, which the range check drops.
    template <int ACT, bool RES>
    __device__ __forceinline__ void store(const Regs &rg, float *y, int64_t ldy, const float *res, int64_t ldr, int Ho, int Wo, int Cout, int b, int oy0,
                                          int ox0) {
        const int64_t opix = (int64_t)Ho * Wo;       // (descriptors per image: byte offsets stay inside one image's output)
        const __amdgpu_buffer_rsrc_t yr = mydet_rsrc(y + b * opix * ldy, opix * ldy * 4);
        const __amdgpu_buffer_rsrc_t rr = mydet_rsrc(RES ? res + b * opix * ldr : y, opix * (RES ? ldr : ldy) * 4);
        const unsigned ldy4 = (unsigned)ldy * 4u, ldr4 = (unsigned)ldr * 4u;
        const int n = nch;
        const bool nok = n < Cout;
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            const int oyb = oy0 + wm * (TM * RPB) + i * RPB;     // first output row of the block
            float rv[16];
            unsigned off_y[16], off_r[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int dr = (r & 3) + 8 * (r >> 2) + 4 * fh;
                const int oy = oyb + (dr >> TWL), ox = ox0 + (dr & (TW - 1));
                const bool ok = nok && oy < Ho && ox < Wo;
                const unsigned pix = (unsigned)(oy * Wo + ox);
                off_y[r] = ok ? pix * ldy4 + (unsigned)n * 4u : P3_OOB;
                off_r[r] = ok ? pix * ldr4 + (unsigned)n * 4u : P3_OOB;
                if (RES) rv[r] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rr, off_r[r], 0, 0));
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                float v = rg.acc[i][r] * pscl + psft;
                if (ACT == MYDET_ACT_LEAKY) v = v > 0.0f ? v : v * 0.1f;
                if (ACT == MYDET_ACT_SWISH) v = v * mydet_sigmoid_fast(v);
                if (RES) v += rv[r];
                __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), yr, off_y[r], 0, 0);
            }
        }
    }
};

}  // namespace
