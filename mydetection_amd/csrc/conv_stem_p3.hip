// Darknet-53's first two layers as ONE launch: 3x3 stem (3 -> 32, stride 1) + 3x3 stride-2 conv (32 -> Cout), both with folded BN
// and activation, float32-exact split-bf16 operands on v_mfma_f32_32x32x16_bf16.
//
// conv_stem_kernel (conv_stem.hip) writes the 32-channel full-resolution map -- the largest tensor of the network -- and
// conv_p3_kernel<2, 64, 0> (conv_p3.hip) reads it straight back.  Here the workgroup of conv_p3's SHAPE-0 stride-2 tile (8 x 16 output
// pixels x 64 channels, 4 waves, same grid, same patch layout, same K loop, same epilogue) computes the 17 x 33-pixel stem patch it
// needs itself, on the matrix pipe, into the LDS patch the nine taps read: the stem map never exists in memory.
//
// Stem phase.  The tile's 19 x 35 x 3 image patch is read through the image's own strides (NCHW as is; outside the image: 0) into
// LDS as float32, planar.  The stem is the GEMM  D[channel 32][pixel 561 -> 18 blocks of 32] = W[32][K 27 -> 32] x P[K][pixel],
// k = (kh, kw, c): the WEIGHTS are the MFMA's A operand (pre-split planes of mydet_split_bf16_f32, Cout 32, K padded to 32 with zeros,
// six 16-byte fragment loads per lane and tile), the PIXELS its B operand -- a lane gathers its pixel's 16 k-values of its k-half
// from the LDS image (consecutive lanes = consecutive pixels: conflict-free), cuts each into three bf16 pieces in registers, and
// the result arrives with lane = pixel, register quad = 4 consecutive channels: exactly the 8-byte units of the patch planes
// (12 ds_write_b64 per 32 pixels).  Patch pixels outside the stem map are the SECOND conv's zero padding: exactly 0, not act(shift).
//
// LDS / occupancy.  One slab (16 channels) of the patch is 3 x 17 x 36 x 32 B = 58 752 B; both slabs + the image would be 125.7 KB:
// one workgroup per CU.  conv_p3 runs two (launch bounds (256, 2): MFMAs of one workgroup under the staging of the other), so this
// kernel keeps that: ONE slab resident (58 752 + 8 208 B image = 66 960 B, two workgroups = 133 920 B of the CU's 160 KB) and the
// stem result of channels 16..31 -- 40 floats per lane -- waits in REGISTERS while the nine taps of slab 0 run, then is split into
// the same buffer (one barrier pair, as conv_p3's slab refresh).  Nothing is recomputed and nothing is re-read from memory.
//
// Arithmetic.  Stem: six piece products per k-step, small ones first, float32 accumulation, then acc * scale + shift and the
// activation as conv_stem_kernel's epilogue (its fmaf chain over the 27 taps becomes the MFMA's sum: equal to float32 round-off).
// Main: conv_p3_kernel's, bit for bit the same order.  Both held to 2e-5 * max|y| against float64 (tests/test_gpu_stem_p3.py).
// Replaces netlist[0] + netlist[1] of models/backbones.py:14-30 (two ATen conv2d / batch_norm / leaky_relu chains, models/modules.py:76-95).
#include "p3_tile.h"

namespace {

typedef P3Geom<2, 0> SPG;                        // conv_p3's stride-2 8 x 16 tile
constexpr int SP_PH = SPG::PH, SP_PW = SPG::PW;
constexpr int SP_NPIX = SP_PH * SP_PW;           // 561 stem pixels per tile
constexpr int SP_NBLK = (SP_NPIX + 31) / 32;     // 18 blocks of 32 pixels
constexpr int SP_BPW = (SP_NBLK + 3) / 4;        // blocks per wave (waves 0, 1: 5; waves 2, 3: 4)
constexpr int SP_SLAB = SPG::LDS;                // 58 752 B
constexpr int SP_IH = SP_PH + 2, SP_IW = SP_PW + 2, SP_ILD = 36;       // image patch, LDS row length
constexpr int SP_ICH = SP_IH * SP_ILD;           // floats per image channel in LDS
constexpr int SP_LDS = SP_SLAB + 3 * SP_ICH * 4; // 66 960 B

struct StemP3Args {
    const float *x, *scale0, *shift0, *scale, *shift;
    const unsigned short *w0, *wsplit;
    float *y;
    int64_t sxb, sxc, sxh, sxw, ldy;
    int B, H, W, pad_t, pad_l, Hs, Ws, act0, Cout, Ho, Wo;
    int tx_n, ntn, nblk, tiles_img;
};

template <int ACT>
__global__ __launch_bounds__(256, 2) void conv_stem_p3_kernel(const StemP3Args p) {
    extern __shared__ __attribute__((aligned(16))) char smem_sp[];
    char *patch = smem_sp;
    float *img = reinterpret_cast<float *>(smem_sp + SP_SLAB);

    const int id = mydet_xcd_remap(blockIdx.x, p.nblk);
    const int nt = id % p.ntn, t = id / p.ntn;
    const int b = t / p.tiles_img, rt = t - b * p.tiles_img;
    const int ty = rt / p.tx_n, tx = rt - ty * p.tx_n;
    const int oy0 = ty * 8, ox0 = tx * 16, n0 = nt * 64;
    const int sy0 = 2 * oy0 - 1, sx0 = 2 * ox0 - 1;                     // stem-map coordinates of the patch origin
    const int tid = threadIdx.x;
    P3Main<2, 64, 0> mp(tid);                                            // conv_p3's BN = 64 roles: waves = 2 row groups x 2 column blocks
    const int wave = mp.wave, fr = mp.fr, fh = mp.fh;

    // ---- image patch -> LDS (float32, planar, rows of SP_ILD)
    {
        const float *xb = p.x + (int64_t)b * p.sxb;
        const int iy0 = sy0 - p.pad_t, ix0 = sx0 - p.pad_l;
        constexpr int NE = 3 * SP_IH * SP_IW, NI = (NE + 255) / 256;
        float v[NI];
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const int e = tid + 256 * i;
            const int c = e / (SP_IH * SP_IW), rem = e - c * (SP_IH * SP_IW);
            const int r = rem / SP_IW, q = rem - r * SP_IW;
            const int iy = iy0 + r, ix = ix0 + q;
            const bool ok = e < NE && (unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W;
            v[i] = ok ? xb[c * p.sxc + (int64_t)iy * p.sxh + (int64_t)ix * p.sxw] : 0.0f;
        }
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const int e = tid + 256 * i;
            const int c = e / (SP_IH * SP_IW), rem = e - c * (SP_IH * SP_IW);
            const int r = rem / SP_IW, q = rem - r * SP_IW;
            if (e < NE) img[c * SP_ICH + r * SP_ILD + q] = v[i];
        }
    }

    const unsigned unit = p3_b_unit(fr, fh);
    mp.weights(p.wsplit, p.Cout, 2, n0);

    float keep[SP_BPW][8];                           // stem channels 16 .. 31 of the wave's pixels, until slab 0's taps are done
    {
        // stem weights (32 rows: block 0 of planes padded to P3_COUT_PAD rows), two k-steps x three planes
        const __amdgpu_buffer_rsrc_t w0r = mydet_rsrc(p.w0, (int64_t)2 * 3 * P3_COUT_PAD * 32);
        bf16x8 wf[2][3];
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
#pragma unroll
            for (int pl = 0; pl < 3; ++pl)
                wf[ks][pl] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(w0r, unit, (ks * 3 + pl) * P3_COUT_PAD * 32, 0));
        // the lane's channels: register r of the accumulator = channel (r & 3) + 8 (r >> 2) + 4 fh
        float sc0[16], sh0[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int ch = (r & 3) + 8 * (r >> 2) + 4 * fh;
            sc0[r] = p.scale0 ? p.scale0[ch] : 1.0f;
            sh0[r] = p.shift0 ? p.shift0[ch] : 0.0f;
        }
        // the lane's k values: k-step ks, element e = k 16 ks + 8 fh + e = (tap k / 3, channel k % 3); k >= 27 is padding
        int koff[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int ka = 16 * (j >> 3) + (j & 7), kb = ka + 8;
            const int ta = ka / 3, tb = kb / 3;
            const int oa = (ka - 3 * ta) * SP_ICH + (ta / 3) * SP_ILD + ta % 3;
            const int ob = kb < 27 ? (kb - 3 * tb) * SP_ICH + (tb / 3) * SP_ILD + tb % 3 : 0;
            koff[j] = fh ? ob : oa;
        }
        __syncthreads();                             // the image patch is in LDS

#pragma unroll
        for (int bi = 0; bi < SP_BPW; ++bi) {
            const int blk = wave + 4 * bi;
            if (blk < SP_NBLK) {                     // (uniform per wave)
                const int m_raw = blk * 32 + fr;
                const bool mok = m_raw < SP_NPIX;
                const int m = mok ? m_raw : SP_NPIX - 1;
                const int py = m / SP_PW, px = m - py * SP_PW;
                const float *ib = img + py * SP_ILD + px;
                bf16x8 pa[2][3];
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    float v = ib[koff[j]];
                    if (j >= 11 && fh) v = 0.0f;     // k 27 .. 31
                    __bf16 h0, h1, h2;
                    split3(v, h0, h1, h2);
                    pa[j >> 3][0][j & 7] = h0; pa[j >> 3][1][j & 7] = h1; pa[j >> 3][2][j & 7] = h2;
                }
                f32x16 acc;
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
                for (int ks = 0; ks < 2; ++ks)
#pragma unroll
                    for (int tt = 0; tt < 6; ++tt)
                        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf[ks][SPLIT_PB[tt]], pa[ks][SPLIT_PA[tt]], acc, 0, 0, 0);     // (pixel piece PA, weight piece PB)
                // folded BN + activation; a pixel outside the stem map is the second conv's padding: 0
                const int sy = sy0 + py, sx = sx0 + px;
                const bool inside = (unsigned)sy < (unsigned)p.Hs && (unsigned)sx < (unsigned)p.Ws;
                const int pos = p3_pos<2, 0>(py, px), sig = p3_pix_sigma<2, 0>(py, px);
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    f32x4 o;                         // four consecutive channels: quad fh of half g & 1 of slab g >> 1
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int r = 4 * g + e;
                        o[e] = inside ? mydet_act(acc[r] * sc0[r] + sh0[r], p.act0) : 0.0f;
                    }
                    if (g < 2) {
                        if (mok) p3_store_quad<2, 0>(patch, p3_quad_off(pos, sig, g & 1, fh), o);
                    } else {
#pragma unroll
                        for (int e = 0; e < 4; ++e) keep[bi][(g - 2) * 4 + e] = o[e];
                    }
                }
            }
        }
    }

    // ---- main phase (p3_tile.h) over the resident slab
    P3Main<2, 64, 0>::Regs rg;
    mp.rows(rg, p.scale, p.shift, p.Cout, n0);
    constexpr int TM = P3Main<2, 64, 0>::TM, ROWLEN = SPG::ROWLEN, PJ0 = SPG::PJ0, PLANE_P = SPG::PLANE, ROWB = P3_ROWB;
    const int oxl = mp.oxl;
    auto load_b = [&](int cs, int tap, bf16x8 (&brg)[3]) {             // conv_p3.hip's, nsl = 2
        const unsigned kt = (unsigned)(tap * 2 + cs);
#pragma unroll
        for (int pl = 0; pl < 3; ++pl)
            brg[pl] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(mp.wr, cs < 2 ? mp.boff : P3_OOB,
                                                     __builtin_amdgcn_readfirstlane(kt * mp.slab_bytes + (unsigned)pl * mp.plane_bytes), 0));
    };
    auto compute = [&](int tap, const bf16x8 (&bf)[3]) {                // conv_p3.hip's, S = 2, SHAPE 0
        const int kh = tap / 3, kw = tap - kh * 3;
        bf16x8 af[TM][3];
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            const int pos = rg.apos[i] + kh * ROWLEN + (kw & 1) * PJ0 + (kw >> 1);
            const int sig = p3_sigma<0>(rg.apy[i] + kh, oxl + (kw >> 1));
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
    load_b(0, 0, rg.breg[0]);
    load_b(0, 1, rg.breg[1]);
    load_b(0, 2, rg.breg[2]);
#pragma unroll
    for (int cs = 0; cs < 2; ++cs) {
        if (cs == 1) {
            mydet_lds_barrier();                     // every wave is done with slab 0's patch
#pragma unroll
            for (int bi = 0; bi < SP_BPW; ++bi) {
                const int m = (wave + 4 * bi) * 32 + fr;
                if (m < SP_NPIX) {
                    const int py = m / SP_PW, px = m - py * SP_PW;
                    const int pos = p3_pos<2, 0>(py, px), sig = p3_pix_sigma<2, 0>(py, px);
#pragma unroll
                    for (int g = 0; g < 2; ++g) {
                        const f32x4 o = {keep[bi][4 * g], keep[bi][4 * g + 1], keep[bi][4 * g + 2], keep[bi][4 * g + 3]};
                        p3_store_quad<2, 0>(patch, p3_quad_off(pos, sig, g, fh), o);
                    }
                }
            }
        }
        mydet_lds_barrier();
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            compute(tap, rg.breg[tap % 3]);
            const int t3 = tap + 3;
            load_b(cs + t3 / 9, t3 % 9, rg.breg[tap % 3]);
        }
    }
    mp.template store<ACT, false>(rg, p.y, p.ldy, nullptr, 0, p.Ho, p.Wo, p.Cout, b, oy0, ox0);
}

template <int ACT>
int sp_launch(const StemP3Args &p, hipStream_t st) {
    static unsigned long long mask = 0;
    auto kern = &conv_stem_p3_kernel<ACT>;
    const int rc = mydet_lds_opt_in(mask, kern, SP_LDS);         // 66 960 B: above the 64 KiB default
    if (rc != 0) return rc;
    hipLaunchKernelGGL(kern, dim3(p.nblk), dim3(256), SP_LDS, st, p);
    return mydet_launch_status();
}

}  // namespace

extern "C" int mydet_conv_stem_p3_lds_bytes(void) { return SP_LDS; }

extern "C" int mydet_conv_stem_p3_f32(const float *x, int64_t sxb, int64_t sxc, int64_t sxh, int64_t sxw, const uint16_t *w0_planes,
                                      const float *scale0, const float *shift0, int act0, const uint16_t *w1_planes, const float *scale1,
                                      const float *shift1, int act1, float *y, int64_t ldy, int B, int H, int W, int C0, int Cout,
                                      int stride0, int pad_t, int pad_l, int Hs, int Ws, int stride1, void *stream) {
    if (!x || !w0_planes || !w1_planes || !y || B <= 0 || H <= 0 || W <= 0 || Hs <= 0 || Ws <= 0 || Cout <= 0) return MYDET_E_BADARG;
    if (C0 != 32 || (Cout & 63) || stride0 != 1 || stride1 != 2) return MYDET_E_UNSUPP;
    if ((act0 != MYDET_ACT_NONE && act0 != MYDET_ACT_LEAKY) || (act1 != MYDET_ACT_NONE && act1 != MYDET_ACT_LEAKY)) return MYDET_E_UNSUPP;
    if ((ldy & 3) || ldy < Cout || ((uintptr_t)y & 15)) return MYDET_E_BADARG;
    if (((uintptr_t)w0_planes & 15) || ((uintptr_t)w1_planes & 15) || ((uintptr_t)x & 3)) return MYDET_E_BADARG;
    StemP3Args p;
    p.x = x; p.scale0 = scale0; p.shift0 = shift0; p.scale = scale1; p.shift = shift1; p.w0 = w0_planes; p.wsplit = w1_planes; p.y = y;
    p.sxb = sxb; p.sxc = sxc; p.sxh = sxh; p.sxw = sxw; p.ldy = ldy;
    p.B = B; p.H = H; p.W = W; p.pad_t = pad_t; p.pad_l = pad_l; p.Hs = Hs; p.Ws = Ws; p.act0 = act0; p.Cout = Cout;
    p.Ho = (Hs - 1) / 2 + 1; p.Wo = (Ws - 1) / 2 + 1;
    // 32-bit byte offsets inside the kernel, relative to the workgroup's image: one image's output stays below 2 GB
    if ((int64_t)p.Ho * p.Wo * ldy * 4 > 0x7FFFFFF0ll) return MYDET_E_UNSUPP;
    const P3Plan pl = mydet_p3_plan(p.Ho, p.Wo, Cout, 2, false);       // ragged 8 x 16 tiles whatever the width: no strip tiles
    p.tx_n = pl.tx_n; p.ntn = Cout / 64;
    p.tiles_img = pl.tiles_img;
    const int64_t nblk = (int64_t)B * p.tiles_img * p.ntn;
    if (nblk > 0x7FFFFFFF || nblk <= 0) return MYDET_E_UNSUPP;
    p.nblk = (int)nblk;
    hipStream_t st = (hipStream_t)stream;
    return act1 == MYDET_ACT_LEAKY ? sp_launch<MYDET_ACT_LEAKY>(p, st) : sp_launch<MYDET_ACT_NONE>(p, st);
}
