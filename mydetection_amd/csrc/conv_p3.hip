// 3x3 convolution (pad 1, stride 1 or 2) with float32-exact split-bf16 operands and an LDS-RESIDENT INPUT PATCH (round 6).
//
// conv_igemm_b3_kernel (conv_igemm.hip) gathers, for every one of the 9 taps, the tile's 128 x 16 activations from global
// memory, cuts them into three bfloat16 pieces and stages them: every input element is loaded and split once per tap that
// uses it -- 2.25 times for a stride-2 layer, 9 times for a stride-1 layer -- and that staging, not the matrix pipe, bounds
// the launch (stride-2 128->256 @160^2: 0.36 ms of 0.66 are staging alone; profiles/HISTORY.md, round 5).
// Here a workgroup owns a SPATIAL tile of TH x TW = 8 x 16 output pixels (128 MFMA rows; 16 x 8 / 32 x 4 strip tiles for the remainder
// columns of maps that are 16 n + 8 / + 4 pixels wide, same launch) x BN output channels.  Per
// 16-channel slab it loads the tile's input patch (17 x 33 pixels at stride 2, 10 x 18 at stride 1) ONCE, splits it once into
// three bf16 planes in LDS, and the 9 taps read their MFMA A fragments straight out of that patch at a tap-dependent offset --
// no im2col tile is ever written.  The weights come pre-split (mydet_split_bf16_f32: the planes conv_igemm_b3_kernel uses,
// slab kt = tap * Cin/16 + slab) and never touch LDS: a wave owns 32 output channels (all 128 rows of the tile at BN = 128), and
// its MFMA B fragment of a (slab, tap, plane) is ONE coalesced 1 KB load -- the planes store each 32-row block as the 64 16-byte
// units of exactly that fragment -- requested three taps ahead.  So the only workgroup barriers are the two around the patch
// refresh of a slab (the first form staged the weights through LDS: two barriers per tap, waves waiting 57 % of their cycles).
//   global loads + split arithmetic per output pixel and slab: 561 / 128 = 4.4 pixels (stride 2; 9 before), 180 / 128 = 1.4
//   (stride 1; 9 before).
// Patch geometry and layout, the main phase over a resident slab and the epilogue are p3_tile.h's (shared with conv_stem_p3.hip); this
// file keeps the refresh of the patch from global memory, the launch and the tile plan.
// Arithmetic: exactly conv_igemm_b3_kernel's (six piece products per k-step, small ones first, float32 accumulation), but
// the K order is (slab, tap) instead of (tap, slab): results agree to float32 round-off, both are held to 2e-5 * max|y|
// against float64 (tests/test_gpu_kernels.py).
// Replaces the ATen conv2d / batch_norm / leaky_relu chain of models/modules.py:76-95 for the stride-2 layers of
// models/backbones.py:14-30 and the 32 -> 64 layer of the first DarkBlock.
#include <cstdlib>

#include "p3_tile.h"

namespace {

struct P3Args {
    const float *x, *scale, *shift, *res;
    const unsigned short *wsplit;
    float *y;
    int64_t ldx, ldr, ldy;
    int B, H, W, Cin, Cout, Ho, Wo;
    int tx_n, ty_n, ntn, nblk;                   // 8 x 16 tiles per image row / column, channel tiles, workgroups
    int main_tiles, tiles_img;                   // tx_n * ty_n; + the strip tiles of the remainder columns (STRIP != 0)
};

// One tile: image b, output rows oy0.., columns ox0.., output channels n0...  S: stride.  BN: output channels per workgroup (64 | 128).
template <int S, int BN, int SHAPE, int ACT, bool RES>
__device__ __forceinline__ void p3_tile(const P3Args &p, char *patch, const int b, const int oy0, const int ox0, const int n0) {
    typedef P3Geom<S, SHAPE> G;
    constexpr int PW = G::PW, ROWLEN = G::ROWLEN, PJ0 = G::PJ0, NPOS = G::NPOS;
    constexpr int NCH = (NPOS * 4 + 255) / 256;      // 16-byte float4 chunks of the patch per thread and slab

    const int tid = threadIdx.x;
    const int iy0 = oy0 * S - 1, ix0 = ox0 * S - 1;
    P3Main<S, BN, SHAPE> m(tid);
    typename P3Main<S, BN, SHAPE>::Regs rg;

    // ---- descriptors.  x: the buffer starts one row + one pixel before image b, so that a patch origin of (-1, -1) is a
    // non-negative offset (the range check sees the voffset only; those addresses are masked to OOB below and never touched)
    const int64_t img = (int64_t)p.H * p.W * p.ldx;
    const int64_t lead = (int64_t)(p.W + 1) * p.ldx;
    const __amdgpu_buffer_rsrc_t xr = mydet_rsrc(p.x + b * img - lead, ((p.B - b) * img + lead) * 4);
    const int nsl = p.Cin >> 4;                      // 16-channel slabs
    m.weights(p.wsplit, p.Cout, nsl, n0);

    // ---- patch staging roles: chunk q = tid + 256 i = (position q >> 2, channel quad q & 3)
    unsigned goff[NCH];                              // byte offset of the chunk's pixel (+ quad) in xr, OOB outside the image / padding
    int ldst[NCH];                                   // byte offset of the chunk in a patch plane
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
        const int q = tid + 256 * i, pos = q >> 2, sc = q & 3;
        const int py = pos / ROWLEN, rem = pos - py * ROWLEN;
        int px, sig;
        bool ok = pos < NPOS;
        if (S == 2) {
            const int par = rem >= PJ0 ? 1 : 0, j = rem - par * PJ0;
            px = 2 * j + par;
            sig = p3_sigma<SHAPE>(py, j);
            ok = ok && px < PW && j < (par ? PJ0 - 1 : PJ0);
        } else {
            px = rem;
            sig = p3_sigma<SHAPE>(py, px);
            ok = ok && px < PW;
        }
        const int iy = iy0 + py, ix = ix0 + px;
        ok = ok && (unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W;
        goff[i] = ok ? (unsigned)((((int64_t)iy * p.W + ix) * p.ldx + sc * 4 + lead) * 4) : P3_OOB;
        ldst[i] = pos < NPOS ? p3_quad_off(pos, sig, sc >> 1, sc & 1) : -1;
    }
    m.rows(rg, p.scale, p.shift, p.Cout, n0);

    f32x4 preg[NCH];
    auto load_patch = [&](int cs) {
        const unsigned coff = (unsigned)cs * 64u;    // 16 channels * 4 bytes
#pragma unroll
        for (int i = 0; i < NCH; ++i)
            preg[i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(xr, (goff[i] != P3_OOB && cs < nsl) ? goff[i] + coff : P3_OOB, 0, 0));
    };
    auto store_patch = [&]() {
#pragma unroll
        for (int i = 0; i < NCH; ++i) {
            if (ldst[i] < 0) continue;
            p3_store_quad<S, SHAPE>(patch, ldst[i], preg[i]);
        }
    };

    constexpr int TM = P3Main<S, BN, SHAPE>::TM, PLANE_P = G::PLANE, ROWB = 32;
    const int fh = m.fh, oxl = m.oxl;
    auto load_b = [&](int cs, int tap, bf16x8 (&brg)[3]) {
        const unsigned kt = (unsigned)(tap * nsl + cs);
#pragma unroll
        for (int pl = 0; pl < 3; ++pl)
            brg[pl] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(m.wr, cs < nsl ? m.boff : P3_OOB,
                                                     __builtin_amdgcn_readfirstlane(kt * m.slab_bytes + (unsigned)pl * m.plane_bytes), 0));
    };
    auto compute = [&](int tap, const bf16x8 (&bf)[3]) {
        const int kh = tap / 3, kw = tap - kh * 3;
        bf16x8 af[TM][3];
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            int pos, sig;
            if (S == 2) {
                pos = rg.apos[i] + kh * ROWLEN + (kw & 1) * PJ0 + (kw >> 1);
                sig = p3_sigma<SHAPE>(rg.apy[i] + kh, oxl + (kw >> 1));
            } else {
                pos = rg.apos[i] + kh * ROWLEN + kw;
                sig = p3_sigma<SHAPE>(rg.apy[i] + kh, oxl + kw);
            }
            const char *a = patch + pos * ROWB + ((fh ^ sig) * 16);
#pragma unroll
            for (int pl = 0; pl < 3; ++pl) af[i][pl] = *reinterpret_cast<const bf16x8 *>(a + pl * PLANE_P);
        }
#pragma unroll
        for (int tt = 0; tt < 6; ++tt)
#pragma unroll
            for (int i = 0; i < TM; ++i)
                rg.acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[i][SPLIT_PA[tt]], bf[SPLIT_PB[tt]], rg.acc[i], 0, 0, 0);
    };
    load_patch(0);
    load_b(0, 0, rg.breg[0]);
    load_b(0, 1, rg.breg[1]);
    load_b(0, 2, rg.breg[2]);
    for (int cs = 0; cs < nsl; ++cs) {
        if (cs > 0) __syncthreads();                 // every wave is done with the previous slab's patch
        store_patch();
        load_patch(cs + 1);                          // in flight under the nine taps below
        __syncthreads();
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            compute(tap, rg.breg[tap % 3]);
            const int t3 = tap + 3;
            load_b(cs + t3 / 9, t3 % 9, rg.breg[tap % 3]);
        }
    }
    m.template store<ACT, RES>(rg, p.y, p.ldy, p.res, p.ldr, p.Ho, p.Wo, p.Cout, b, oy0, ox0);
}

// The launch: workgroup id -> (channel tile, image, tile of the image); ids of one spatial tile are neighbours (the patch is shared
// through L2).  STRIP != 0: the image's last tiles are strip tiles (shape STRIP) over the columns behind the tx_n * 16 whole ones.
template <int S, int BN, int STRIP, int ACT, bool RES>
__global__ __launch_bounds__(256, 2) void conv_p3_kernel(const P3Args p) {
    extern __shared__ __attribute__((aligned(16))) char smem_p3[];
    const int id = mydet_xcd_remap(blockIdx.x, p.nblk);
    const int nt = id % p.ntn, t = id / p.ntn;
    const int b = t / p.tiles_img, r = t - b * p.tiles_img;
    if constexpr (STRIP != 0) {
        if (r >= p.main_tiles) {                     // (uniform per workgroup)
            p3_tile<S, BN, STRIP, ACT, RES>(p, smem_p3, b, (r - p.main_tiles) * P3Geom<S, STRIP>::TH, p.tx_n * 16, nt * BN);
            return;
        }
    }
    const int ty = r / p.tx_n, tx = r - ty * p.tx_n;
    p3_tile<S, BN, 0, ACT, RES>(p, smem_p3, b, ty * 8, tx * 16, nt * BN);
}

template <int S, int BN, int STRIP, int ACT, bool RES>
int p3_launch(const P3Args &p, hipStream_t st) {
    constexpr int L0 = P3Geom<S, 0>::LDS, L1 = P3Geom<S, STRIP>::LDS, LDS = L0 > L1 ? L0 : L1;
    static_assert(LDS <= 65536, "dynamic LDS within the default limit: no opt-in");
    hipLaunchKernelGGL((conv_p3_kernel<S, BN, STRIP, ACT, RES>), dim3(p.nblk), dim3(256), LDS, st, p);
    return mydet_launch_status();
}

template <int S, int BN, int STRIP>
int p3_dispatch(const P3Args &p, int act, bool res, hipStream_t st) {
    if (act == MYDET_ACT_LEAKY) return res ? p3_launch<S, BN, STRIP, MYDET_ACT_LEAKY, true>(p, st) : p3_launch<S, BN, STRIP, MYDET_ACT_LEAKY, false>(p, st);
    if (act == MYDET_ACT_NONE) return res ? p3_launch<S, BN, STRIP, MYDET_ACT_NONE, true>(p, st) : p3_launch<S, BN, STRIP, MYDET_ACT_NONE, false>(p, st);
    return MYDET_E_UNSUPP;
}

}  // namespace

// Tile plan (host only; the launcher's, the fused stem launcher's with strips off, and exported as mydet_conv3x3_p3_plan): whole
// 8 x 16 tiles; a remainder of 8 / 4 columns (stride 2) goes to 16 x 8 / 32 x 4 strip tiles of the same launch, any other remainder to
// a ragged last column of 8 x 16 tiles.  Tuning knobs, read from the environment once per process: MYDET_P3_FORM=1 = 64-channel tiles
// whatever Cout (experiments); MYDET_P3_STRIP=0 = always the ragged column (A/B).
P3Plan mydet_p3_plan(int Ho, int Wo, int Cout, int stride, bool strips) {
    static const int form = [] { const char *e = getenv("MYDET_P3_FORM"); return e ? atoi(e) : 0; }();
    static const bool strip_on = [] { const char *e = getenv("MYDET_P3_STRIP"); return !(e && atoi(e) == 0); }();
    P3Plan pl;
    pl.BN = Cout > 64 && form != 1 ? 128 : 64;
    const int rem = Wo & 15;
    pl.strip = (stride == 2 && strips && strip_on) ? (rem == 8 ? 1 : rem == 4 ? 2 : 0) : 0;
    pl.tx_n = pl.strip ? Wo / 16 : (Wo + 15) / 16;
    pl.ty_n = (Ho + 7) / 8;
    pl.ntn = (Cout + pl.BN - 1) / pl.BN;
    pl.main_tiles = pl.tx_n * pl.ty_n;
    pl.tiles_img = pl.main_tiles + (pl.strip == 1 ? (Ho + 15) / 16 : pl.strip == 2 ? (Ho + 31) / 32 : 0);
    const int l0 = stride == 2 ? P3Geom<2, 0>::LDS : P3Geom<1, 0>::LDS;
    const int l1 = pl.strip == 1 ? P3Geom<2, 1>::LDS : pl.strip == 2 ? P3Geom<2, 2>::LDS : 0;
    pl.lds = l0 > l1 ? l0 : l1;
    return pl;
}

/* Test hook (host only, no GPU call): the tile plan mydet_conv3x3_p3_f32 launches for an Ho x Wo output map (include/mydet.h). */
extern "C" int mydet_conv3x3_p3_plan(int Ho, int Wo, int Cout, int stride, int32_t *out) {
    if (!out || Ho <= 0 || Wo <= 0 || Cout <= 0 || (int64_t)Ho * Wo > (int64_t)1 << 30) return MYDET_E_BADARG;
    if (stride != 1 && stride != 2) return MYDET_E_UNSUPP;
    const P3Plan pl = mydet_p3_plan(Ho, Wo, Cout, stride, true);
    out[0] = pl.BN; out[1] = pl.strip; out[2] = pl.tx_n; out[3] = pl.ty_n;
    out[4] = pl.main_tiles; out[5] = pl.tiles_img; out[6] = pl.ntn; out[7] = pl.lds;
    return 0;
}

extern "C" int mydet_conv3x3_p3_f32(const float *x, int64_t ldx, const uint16_t *w_planes, const float *scale, const float *shift,
                                    const float *residual, int64_t ldr, float *y, int64_t ldy, int B, int H, int W, int Cin, int Cout,
                                    int stride, int act, void *stream) {
    if (!x || !w_planes || !y || B <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0) return MYDET_E_BADARG;
    if ((stride != 1 && stride != 2) || (Cin & 15) || (ldx & 3) || ldx < Cin || ldy < Cout || (residual && ldr < Cout)) return MYDET_E_UNSUPP;
    if (((uintptr_t)x & 15) || ((uintptr_t)w_planes & 15)) return MYDET_E_BADARG;
    P3Args p;
    p.x = x; p.scale = scale; p.shift = shift; p.res = residual; p.wsplit = w_planes; p.y = y;
    p.ldx = ldx; p.ldr = ldr; p.ldy = ldy;
    p.B = B; p.H = H; p.W = W; p.Cin = Cin; p.Cout = Cout;
    p.Ho = (H + 2 - 3) / stride + 1; p.Wo = (W + 2 - 3) / stride + 1;
    // 32-bit byte offsets inside the kernel, relative to the workgroup's image: one image's input and output stay below 2 GB
    if ((int64_t)(H + 1) * (W + 1) * ldx * 4 > 0x7FFFFFF0ll || (int64_t)p.Ho * p.Wo * (ldy > ldr ? ldy : ldr) * 4 > 0x7FFFFFF0ll) return MYDET_E_UNSUPP;
    const P3Plan pl = mydet_p3_plan(p.Ho, p.Wo, Cout, stride, true);
    const bool wide = pl.BN == 128;
    const int strip = pl.strip;
    p.tx_n = pl.tx_n; p.ty_n = pl.ty_n; p.ntn = pl.ntn; p.main_tiles = pl.main_tiles; p.tiles_img = pl.tiles_img;
    const int64_t nblk = (int64_t)B * p.tiles_img * p.ntn;
    if (nblk > 0x7FFFFFFF || nblk <= 0) return MYDET_E_UNSUPP;
    p.nblk = (int)nblk;
    hipStream_t st = (hipStream_t)stream;
    const bool res = residual != nullptr;
    if (stride == 2) {
        if (strip == 1) return wide ? p3_dispatch<2, 128, 1>(p, act, res, st) : p3_dispatch<2, 64, 1>(p, act, res, st);
        if (strip == 2) return wide ? p3_dispatch<2, 128, 2>(p, act, res, st) : p3_dispatch<2, 64, 2>(p, act, res, st);
        return wide ? p3_dispatch<2, 128, 0>(p, act, res, st) : p3_dispatch<2, 64, 0>(p, act, res, st);
    }
    return wide ? p3_dispatch<1, 128, 0>(p, act, res, st) : p3_dispatch<1, 64, 0>(p, act, res, st);
}
