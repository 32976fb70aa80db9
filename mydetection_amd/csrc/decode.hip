// Box decode of one pyramid level: raw head logits -> (cxcywh box, class index, score).
//
// HBM-bound: every head logit is read once (8.57 MB/image for YOLOv3-80 @640^2) and 28 B are written per
// candidate.  A workgroup stages a tile of PIX consecutive pixels (all anchors, all channels) from HBM into LDS
// with coalesced 16-byte loads -- the pixel-major head rows are contiguous in memory -- into rows padded to an
// odd number of floats, so that in the compute phase, where a THREAD owns one candidate (pixel, anchor) and walks
// its 80 class logits, the 64 lanes of a wave (64 different pixels, same channel) hit 64 different banks.
// The class max / first argmax is torch.max over the float32 sigmoids: a strict-greater scan of the logits finds the
// best and the runner-up logit, and where the float32 logistic merges the two (neighbouring float32 logits share one
// float32 sigmoid from about -2 up, where the logistic's slope shrinks a logit ulp below the ulp of its value) the
// sigmoid values decide and the first index among equal ones wins.  Box arithmetic follows the reference's operation
// order; the file is built with -ffp-contract=off so no product is fused into a sum.  Outputs of a wave are 64 consecutive
// candidates: coalesced 16-byte box stores.  All pyramid levels are decoded by ONE launch (a tile belongs to a
// level), and a workgroup prefetches its next tile into registers while it computes the current one.
//
//   YOLO   models/detlayers/yolov3.py:41-69    cx=(s(tx)+x)*stride, w=exp(tw)*aw, score=s(conf)*max s(cls)
//   RETINA models/detlayers/retinanet.py:63-82 cx=acx+tx*aw, w=exp(tw)*aw, clamp [1,max(H,W)], score=max s(cls)
//   FCOS   models/detlayers/fcos2.py:222-251   ltrb=exp(t)*stride, clamp to image, score=sqrt(s(conf)*max s(cls))
//   RAPID  models/detlayers/rapid.py:36-81     YOLO box + deg=((s(t4)*2*pi-pi)/pi)*180, score=s(conf) (C == 0) or
//                                               sqrt(s(conf)*max s(cls)); 5-float rows (20 B): a wave's 64 candidates
//                                               are one contiguous 1280-byte run written as dword stores
//   UV5    models/detlayers/uv5.py:42-91       s=s(t[0..3]), cx=(s0*2-0.5+x)*stride, w=(s2*2)^2*aw, score as YOLO; no
//                                               clamp: cx >= -stride/2, w <= 4*aw.  Not a value of the public `mode`
//                                               argument (which ends at RAPID): mydet_decode_uv5_levels_f32 selects it
#include <cstdlib>

#include "common.h"

namespace {

constexpr int MAX_A = 16;
constexpr int DECODE_UV5 = MYDET_DECODE_RAPID + 1;       // internal: reached through its own entry point only
constexpr int MAX_LEVELS = 5;
constexpr int MAXV = 12;          // float4 staging registers per thread (one tile = at most MAXV * 256 float4)

struct Level {
    const float *box, *cls;
    int64_t ldbox, ldcls, n_off, npix;
    int H, W, tile0, ntiles;
    float stride;
    float aw[MAX_A], ah[MAX_A];
};

struct DecodeArgs {
    int mode, nlevels, total_tiles;
    int box_astride, box_c0, cls_astride, cls_c0, conf_c0;
    int A, C, img_h, img_w;
    int box_span, cls_span;      // floats of a pixel actually needed (multiples of 4)
    int same;                    // box and cls are the same tensor
    int PIX, row;                // pixels per tile, LDS row length (odd)
    int tpc;                     // threads per candidate: 1, 2 or 4 (tiles with <= 128 / <= 64 candidates: single-anchor heads)
    unsigned qc, qb, mc, mb;     // float4 per row (cls, box) and their magic reciprocals: i / q == (i * m) >> 20
    float *bbox;
    int64_t *cidx;
    float *score;
    int64_t N;
    Level lv[MAX_LEVELS];
};

// Staging is branch-free so the loads of a tile are all in flight together: indices past the tile are clamped
// (they re-load the last element) and their LDS stores are diverted to a dump slot behind the tile.
constexpr int MAXV_B = 2;         // float4 per thread for the box rows when they live in a separate tensor

template <int NV, int NVB>
__device__ __forceinline__ void tile_load(const DecodeArgs &p, const Level &L, int tile, f32x4 (&v)[NV],
                                          f32x4 (&vb)[NVB ? NVB : 1]) {
    const int64_t pix0 = (int64_t)tile * p.PIX;
    const int npx = (int)(L.npix - pix0 < p.PIX ? L.npix - pix0 : p.PIX);
    const unsigned ncls4 = npx * p.qc, nbox4 = npx * p.qb;
    const float *cls = L.cls + pix0 * L.ldcls, *box = L.box + pix0 * L.ldbox;
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        unsigned i = threadIdx.x + 256u * j;
        i = i < ncls4 ? i : ncls4 - 1;
        const unsigned r = (i * p.mc) >> 20, c4 = i - r * p.qc;
        v[j] = __builtin_nontemporal_load(reinterpret_cast<const f32x4 *>(cls + (int64_t)r * L.ldcls + c4 * 4));      // read once
    }
#pragma unroll
    for (int j = 0; j < NVB; ++j) {
        unsigned i = threadIdx.x + 256u * j;
        i = i < nbox4 ? i : nbox4 - 1;
        const unsigned r = (i * p.mb) >> 20, c4 = i - r * p.qb;
        vb[j] = __builtin_nontemporal_load(reinterpret_cast<const f32x4 *>(box + (int64_t)r * L.ldbox + c4 * 4));
    }
}

// Registers -> LDS rows of odd length (4 dword writes per float4: the rows are not 16-byte aligned).
template <int NV, int NVB>
__device__ __forceinline__ void tile_store(const DecodeArgs &p, int npx, const f32x4 (&v)[NV],
                                           const f32x4 (&vb)[NVB ? NVB : 1], float *sm) {
    const unsigned ncls4 = npx * p.qc, nbox4 = npx * p.qb;
    float *dump = sm + p.PIX * p.row;
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        const unsigned i = threadIdx.x + 256u * j;
        const unsigned r = (i * p.mc) >> 20, c4 = i - r * p.qc;
        float *d = i < ncls4 ? sm + r * p.row + c4 * 4 : dump;
        d[0] = v[j][0]; d[1] = v[j][1]; d[2] = v[j][2]; d[3] = v[j][3];
    }
#pragma unroll
    for (int j = 0; j < NVB; ++j) {
        const unsigned i = threadIdx.x + 256u * j;
        const unsigned r = (i * p.mb) >> 20, c4 = i - r * p.qb;
        float *d = i < nbox4 ? sm + r * p.row + p.cls_span + c4 * 4 : dump;
        d[0] = vb[j][0]; d[1] = vb[j][1]; d[2] = vb[j][2]; d[3] = vb[j][3];
    }
}

// grid = (tile slots, levels): blockIdx.y picks the level ONCE (static-index select chain, no dynamic indexing of
// the kernel arguments), blockIdx.x strides over that level's tiles; surplus workgroups of small levels exit.
// NV / NVB: float4 staging registers per thread for the class rows / the separate box rows (0 when box == cls);
// compile-time so the prefetch of a tile is one straight-line run of loads, all in flight together.
template <int NV, int NVB>
__global__ __launch_bounds__(256) void decode_kernel(const DecodeArgs p) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    __shared__ float s_aw[MAX_A], s_ah[MAX_A];
    const int l = blockIdx.y;
    Level L = p.lv[0];
#pragma unroll
    for (int k = 1; k < MAX_LEVELS; ++k)
        if (l == k) L = p.lv[k];
    if ((int)blockIdx.x >= L.ntiles) return;
#pragma unroll
    for (int a = 0; a < MAX_A; ++a)
        if (threadIdx.x == a) { s_aw[a] = L.aw[a]; s_ah[a] = L.ah[a]; }
    const float fmaxhw = (float)(p.img_h > p.img_w ? p.img_h : p.img_w);
    const int box_col = p.same ? 0 : p.cls_span;
    const int hw = L.H * L.W;
    const float st = L.stride;
    f32x4 v[NV], vb[NVB ? NVB : 1];
    tile_load<NV, NVB>(p, L, blockIdx.x, v, vb);
    for (int tile = blockIdx.x; tile < L.ntiles; tile += gridDim.x) {
        const int64_t pix0 = (int64_t)tile * p.PIX;
        const int npx = (int)(L.npix - pix0 < p.PIX ? L.npix - pix0 : p.PIX);
        tile_store<NV, NVB>(p, npx, v, vb, sm);
        __syncthreads();
        if (tile + (int)gridDim.x < L.ntiles)                  // flies under the compute phase
            tile_load<NV, NVB>(p, L, tile + gridDim.x, v, vb);
        // tpc > 1: tpc neighbouring lanes share candidate c -- each scans its share of the classes, lane exchanges pick the
        // winner (a tie goes to the lower share, i.e. the first maximum, as in the sequential scan)
        const int tl = p.tpc == 4 ? 2 : (p.tpc == 2 ? 1 : 0);
        const int part = threadIdx.x & (p.tpc - 1);
        const int cstep = 256 >> tl;
        const int cshare = (p.C + p.tpc - 1) >> tl;
        const int k_lo = part * cshare < p.C ? part * cshare : p.C - 1;
        const int k_hi = k_lo + cshare < p.C ? k_lo + cshare : p.C;
        for (int c = (int)(threadIdx.x >> tl); c < p.PIX * p.A; c += cstep) {
            const int a = c / p.PIX, px = c - a * p.PIX;
            if (px >= npx) continue;                   // (both lanes of a pair leave together)
            const float *rowp = sm + px * p.row;
            const float *cl = rowp + a * p.cls_astride + p.cls_c0;
            // class max / first argmax (strict >: the first maximum wins, as torch.max)
            // ... and the runner-up VALUE (`second`: the largest logit at another index, equal to `best` on an exact tie): it
            // decides below whether the float32 logistic can merge the two
            // C == 0 (RAPiD without classes): no class logit is read, class 0, the score is the objectness alone
            float best = p.C > 0 ? cl[k_lo] : 0.0f, second = -__builtin_inff();
            int bi = p.C > 0 ? k_lo : 0;
            for (int k0 = k_lo + 1; k0 < k_hi; k0 += 8) {      // 8 LDS reads in flight, then the ordered compare chain
                float x[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) x[j] = cl[k0 + j < k_hi ? k0 + j : k_hi - 1];   // clamped repeats never win ...
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const bool real = k0 + j < k_hi;           // ... and must not pose as a runner-up either
                    const bool gt = x[j] > best;
                    second = gt ? best : ((real && x[j] > second) ? x[j] : second);
                    bi = gt ? k0 + j : bi;
                    best = gt ? x[j] : best;
                }
            }
            for (int sft = 1; sft < p.tpc; sft <<= 1) {
                const float ob = __shfl_xor(best, sft), os = __shfl_xor(second, sft);
                const int obi = __shfl_xor(bi, sft);
                const bool take = (part & sft) ? !(best > ob) : (ob > best);     // the upper share wins only when strictly greater
                second = fmaxf(fmaxf(second, os), take ? best : ob);             // the loser's best is a runner-up too
                best = take ? ob : best;
                bi = take ? obi : bi;
            }
            // The scan's winner is torch.max's answer exactly when its float32 logistic is strictly above the runner-up's:
            // no class has a logit between `second` and `best`, every other one is <= `second`, and 1 / (1 + expf(-x)) is
            // monotone, so no other class reaches the winner's value.  Otherwise (an exact tie, or two neighbouring logits
            // merged by float32 rounding anywhere from about -2 up) the values decide below.  Where even the best logistic is
            // 0 (every logit below -88.7: expf(-x) overflows) the scan's winner stands: the exact logistics there are distinct
            // float32 denormals down to -103, and the largest logit is their first maximum, as in float64.
            float cmax = p.C == 0 ? 1.0f : mydet_sigmoid(best);
            const bool isolated = p.C == 0 || cmax == 0.0f || mydet_sigmoid(second) < cmax;
            if (!isolated) {                           // rare: compare the sigmoid values themselves
                // ... of the classes that can tie with the best one.  The logistic is monotonic, and a logit two below the best
                // (or below 15 when the best one is past 17, where the float32 logistic is exactly 1) has a float32 logistic
                // at least four ulps smaller: it can neither win nor tie, so its logistic is not evaluated (a wave in which ONE
                // lane is saturated used to pay C logistics per lane: decode 0.059 -> 0.113 ms on a saturating head).
                const float lim = best > -80.0f ? fminf(best - 2.0f, 15.0f) : -__builtin_inff();
                cmax = -1.0f;
                bi = 0;
                for (int k0 = 0; k0 < p.C; k0 += 8) {          // 8 LDS reads in flight, as in the scan above
                    float x[8];
#pragma unroll
                    for (int j = 0; j < 8; ++j) x[j] = k0 + j < p.C ? cl[k0 + j] : -__builtin_inff();
#pragma unroll
                    for (int j = 0; j < 8; ++j)
                        if (x[j] >= lim) {                     // rare: a logistic only for the few classes that can tie
                            const float sv = mydet_sigmoid(x[j]);
                            if (sv > cmax) { cmax = sv; bi = k0 + j; }
                        }
                }
            }
            if (part) continue;                        // lane 2c finishes the candidate
            const float *t = rowp + box_col + a * p.box_astride + p.box_c0;
            const float t0 = t[0], t1 = t[1], t2 = t[2], t3 = t[3];
            const int64_t pix = pix0 + px;
            const int b = (int)(pix / hw);
            const int rem = (int)(pix - (int64_t)b * hw);
            const int gy = rem / L.W, gx = rem - gy * L.W;
            const float aw = s_aw[a], ah = s_ah[a];
            f32x4 o;
            float sc;
            if (p.mode == MYDET_DECODE_YOLO) {
                o[0] = (mydet_sigmoid(t0) + (float)gx) * st;
                o[1] = (mydet_sigmoid(t1) + (float)gy) * st;
                o[2] = expf(t2) * aw;
                o[3] = expf(t3) * ah;
                sc = mydet_sigmoid(rowp[a * p.cls_astride + p.conf_c0]) * cmax;
            } else if (p.mode == DECODE_UV5) {
                // float32 in the reference's operation order: ((s*2 - 0.5) + g) * stride and ((s*2) * (s*2)) * anchor, every
                // operation rounded on its own (tests/test_uv5_host.py restates this order on the reference layer's fixture
                // and matches its boxes bit for bit)
                const float s0 = mydet_sigmoid(t0), s1 = mydet_sigmoid(t1);
                const float s2 = mydet_sigmoid(t2) * 2.0f, s3 = mydet_sigmoid(t3) * 2.0f;
                o[0] = ((s0 * 2.0f - 0.5f) + (float)gx) * st;
                o[1] = ((s1 * 2.0f - 0.5f) + (float)gy) * st;
                o[2] = (s2 * s2) * aw;
                o[3] = (s3 * s3) * ah;
                sc = mydet_sigmoid(rowp[a * p.cls_astride + p.conf_c0]) * cmax;
            } else if (p.mode == MYDET_DECODE_RETINA) {
                const float acx = st * 0.5f + (float)gx * st;
                const float acy = st * 0.5f + (float)gy * st;
                o[0] = acx + t0 * aw;
                o[1] = acy + t1 * ah;
                o[2] = expf(t2) * aw;
                o[3] = expf(t3) * ah;
#pragma unroll
                for (int j = 0; j < 4; ++j) o[j] = fminf(fmaxf(o[j], 1.0f), fmaxhw);
                sc = cmax;
            } else if (p.mode == MYDET_DECODE_RAPID) {
                // float32 in the reference's operation order, and the Python float np.pi acts as the FLOAT32 constant:
                // PyTorch casts a Python scalar to the tensor's dtype (tests/test_rapid_host.py restates this order on the
                // reference layer's fixture and matches its angles bit for bit; the float64-scalar reading does not)
                constexpr float pi = 3.14159265358979323846f;
                o[0] = (mydet_sigmoid(t0) + (float)gx) * st;
                o[1] = (mydet_sigmoid(t1) + (float)gy) * st;
                o[2] = expf(t2) * aw;
                o[3] = expf(t3) * ah;
                const float rad = mydet_sigmoid(t[4]) * 2.0f * pi - pi;
                const float deg = rad / pi * 180.0f;
                const float conf = mydet_sigmoid(rowp[a * p.cls_astride + p.conf_c0]);
                sc = p.C == 0 ? conf : sqrtf(conf * cmax);
                const int64_t n = (int64_t)b * p.N + L.n_off + ((int64_t)a * L.H + gy) * L.W + gx;
                float *d = p.bbox + n * 5;         // 20-byte rows: dword stores, consecutive lanes = consecutive rows
                d[0] = o[0]; d[1] = o[1]; d[2] = o[2]; d[3] = o[3]; d[4] = deg;
                p.cidx[n] = (int64_t)bi;
                p.score[n] = sc;
                continue;
            } else {
                const float cx = (float)gx * st + st * 0.5f;
                const float cy = (float)gy * st + st * 0.5f;
                const float fw = (float)p.img_w, fh = (float)p.img_h;
                const float x1 = fminf(fmaxf(cx - expf(t0) * st, 0.0f), fw);
                const float y1 = fminf(fmaxf(cy - expf(t1) * st, 0.0f), fh);
                const float x2 = fminf(fmaxf(cx + expf(t2) * st, 0.0f), fw);
                const float y2 = fminf(fmaxf(cy + expf(t3) * st, 0.0f), fh);
                o[0] = (x1 + x2) / 2.0f;
                o[1] = (y1 + y2) / 2.0f;
                o[2] = x2 - x1;
                o[3] = y2 - y1;
                sc = sqrtf(mydet_sigmoid(rowp[a * p.cls_astride + p.conf_c0]) * cmax);
            }
            const int64_t n = (int64_t)b * p.N + L.n_off + ((int64_t)a * L.H + gy) * L.W + gx;
            *reinterpret_cast<f32x4 *>(p.bbox + n * 4) = o;
            p.cidx[n] = (int64_t)bi;
            p.score[n] = sc;
        }
        __syncthreads();
    }
}

template <int NV>
void launch_nvb(int needb, dim3 grid, size_t lds, void *stream, const DecodeArgs &p) {
    if (needb == 0) hipLaunchKernelGGL((decode_kernel<NV, 0>), grid, dim3(256), lds, (hipStream_t)stream, p);
    else if (needb == 1) hipLaunchKernelGGL((decode_kernel<NV, 1>), grid, dim3(256), lds, (hipStream_t)stream, p);
    else hipLaunchKernelGGL((decode_kernel<NV, 2>), grid, dim3(256), lds, (hipStream_t)stream, p);
}

unsigned magic20(unsigned q, unsigned max_i) {       // m with (i * m) >> 20 == i / q for all i <= max_i (checked)
    const unsigned m = (1u << 20) / q + 1;
    for (unsigned i = 0; i <= max_i; ++i)
        if (((uint64_t)i * m) >> 20 != i / q || (uint64_t)i * m > 0xFFFFFFFFull) return 0;
    return m;
}

// Argument checks, tile plan and launch of every decode entry point; `mode` is a public MYDET_DECODE_* value or DECODE_UV5.
int decode_levels(int mode, int nlevels, const mydet_decode_level *levels, int box_astride, int box_c0, int cls_astride,
                  int cls_c0, int conf_c0, int A, int C, int B, int img_h, int img_w, float *bbox, int64_t *class_idx,
                  float *score, int64_t N, void *stream) {
    if (mode < 0 || mode > DECODE_UV5 || !levels || nlevels <= 0 || nlevels > MAX_LEVELS || !bbox || !class_idx || !score)
        return MYDET_E_BADARG;
    if (A <= 0 || A > MAX_A || C < (mode == MYDET_DECODE_RAPID ? 0 : 1) || C > 128 || B <= 0 || ((uintptr_t)bbox & 15)) return MYDET_E_BADARG;
    DecodeArgs p;
    p.mode = mode; p.nlevels = nlevels;
    p.box_astride = box_astride; p.box_c0 = box_c0; p.cls_astride = cls_astride; p.cls_c0 = cls_c0;
    p.conf_c0 = conf_c0; p.A = A; p.C = C; p.img_h = img_h; p.img_w = img_w;
    p.bbox = bbox; p.cidx = class_idx; p.score = score; p.N = N;
    int cls_need = (A - 1) * cls_astride + cls_c0 + C;
    if (mode != MYDET_DECODE_RETINA) {
        const int cneed = (A - 1) * cls_astride + conf_c0 + 1;
        cls_need = cls_need > cneed ? cls_need : cneed;
    }
    const int box_need = (A - 1) * box_astride + box_c0 + (mode == MYDET_DECODE_RAPID ? 5 : 4);
    p.same = 1;
    for (int l = 0; l < nlevels; ++l)
        if (levels[l].box != levels[l].cls || levels[l].ldbox != levels[l].ldcls) p.same = 0;
    if (p.same) cls_need = cls_need > box_need ? cls_need : box_need;
    p.cls_span = (cls_need + 3) & ~3;
    p.box_span = (box_need + 3) & ~3;
    p.row = (p.cls_span + (p.same ? 0 : p.box_span)) | 1;               // odd row length: conflict-free column walks
    p.qc = p.cls_span >> 2; p.qb = p.box_span >> 2;
    // 32-pixel tiles (33 KB for YOLO: 4 workgroups per CU), grown while a tile holds fewer candidates than the
    // workgroup has threads (single-anchor heads) and still fits the LDS / staging-register budget
    auto fits = [&](int pix) {
        return (size_t)pix * p.row * sizeof(float) <= 60 * 1024 && (size_t)pix * p.qc <= MAXV * 256 &&
               (p.same || (size_t)pix * p.qb <= MAXV_B * 256);
    };
    p.PIX = 32;
    static const int forced_pix = [] { const char *e = getenv("MYDET_DECODE_PIX"); return e ? atoi(e) : 0; }();      // tuning knob, read once
    if (forced_pix > 0) p.PIX = forced_pix;
    while (p.PIX > 1 && !fits(p.PIX)) p.PIX >>= 1;
    if (!fits(p.PIX)) return MYDET_E_UNSUPP;
    if (!getenv("MYDET_DECODE_PIX"))
        while (p.PIX * A < 256 && fits(p.PIX * 2)) p.PIX <<= 1;
    p.tpc = C < 16 ? 1 : (p.PIX * A <= 64 ? 4 : (p.PIX * A <= 128 ? 2 : 1));
    p.mc = magic20(p.qc, p.PIX * p.qc);
    p.mb = magic20(p.qb, p.PIX * p.qb);
    if (!p.mc || !p.mb) return MYDET_E_UNSUPP;
    int tile0 = 0;
    for (int l = 0; l < MAX_LEVELS; ++l) {
        Level &L = p.lv[l];
        for (int a = 0; a < MAX_A; ++a) { L.aw[a] = 0.f; L.ah[a] = 0.f; }
        if (l >= nlevels) { L = p.lv[0]; L.ntiles = 0; L.tile0 = tile0; continue; }
        const mydet_decode_level &in = levels[l];
        if (!in.box || !in.cls || in.H <= 0 || in.W <= 0 || (in.ldbox & 3) || (in.ldcls & 3) ||
            ((uintptr_t)in.box & 15) || ((uintptr_t)in.cls & 15))
            return MYDET_E_BADARG;
        if (p.cls_span > in.ldcls || p.box_span > in.ldbox) return MYDET_E_BADARG;
        if (mode != MYDET_DECODE_FCOS && !in.anchors_wh) return MYDET_E_BADARG;
        if (in.n_off < 0 || in.n_off + (int64_t)A * in.H * in.W > N) return MYDET_E_BADARG;
        L.box = in.box; L.cls = in.cls; L.ldbox = in.ldbox; L.ldcls = in.ldcls; L.n_off = in.n_off;
        L.H = in.H; L.W = in.W; L.stride = in.stride; L.npix = (int64_t)B * in.H * in.W;
        if (in.anchors_wh)      // HOST pointer: the pairs travel as kernel arguments
            for (int a = 0; a < A; ++a) { L.aw[a] = in.anchors_wh[2 * a]; L.ah[a] = in.anchors_wh[2 * a + 1]; }
        const int64_t nt = (L.npix + p.PIX - 1) / p.PIX;
        if (nt + tile0 > 0x7fffffff) return MYDET_E_BADARG;
        L.tile0 = tile0; L.ntiles = (int)nt;
        tile0 += (int)nt;
    }
    p.total_tiles = tile0;
    const size_t lds = ((size_t)p.PIX * p.row + 4) * sizeof(float);     // + dump slot for clamped staging lanes
    int max_tiles = 0;
    for (int l = 0; l < nlevels; ++l) max_tiles = p.lv[l].ntiles > max_tiles ? p.lv[l].ntiles : max_tiles;
    // one resident round of workgroups per level (256 CUs x workgroups per CU, bounded by LDS): the
    // big level's workgroups then all run concurrently and loop over equal shares of its tiles
    int per_cu = (int)((160 * 1024) / (lds + 512));
    per_cu = per_cu > 3 ? 3 : (per_cu < 1 ? 1 : per_cu);                  // 3 measured best (2: -15 %, 4: -2 %)
    if (const char *e = getenv("MYDET_DECODE_GX")) per_cu = atoi(e);      // tuning knob
    const int resident = 256 * per_cu;
    const int gx = max_tiles < resident ? max_tiles : resident;
    const int need = (int)(((size_t)p.PIX * p.qc + 255) / 256);
    const int needb = p.same ? 0 : (int)(((size_t)p.PIX * p.qb + 255) / 256);
    const dim3 grid((unsigned)gx, (unsigned)nlevels);
    if (need <= 1) launch_nvb<1>(needb, grid, lds, stream, p);
    else if (need <= 2) launch_nvb<2>(needb, grid, lds, stream, p);
    else if (need <= 3) launch_nvb<3>(needb, grid, lds, stream, p);
    else if (need <= 4) launch_nvb<4>(needb, grid, lds, stream, p);
    else if (need <= 6) launch_nvb<6>(needb, grid, lds, stream, p);
    else if (need <= 8) launch_nvb<8>(needb, grid, lds, stream, p);
    else if (need <= 10) launch_nvb<10>(needb, grid, lds, stream, p);
    else launch_nvb<12>(needb, grid, lds, stream, p);
    return mydet_launch_status();
}

}  // namespace

extern "C" int mydet_decode_levels_f32(int mode, int nlevels, const mydet_decode_level *levels, int box_astride,
                                       int box_c0, int cls_astride, int cls_c0, int conf_c0, int A, int C, int B,
                                       int img_h, int img_w, float *bbox, int64_t *class_idx, float *score, int64_t N,
                                       void *stream) {
    if (mode < 0 || mode > MYDET_DECODE_RAPID) return MYDET_E_BADARG;      // the public modes end at RAPID
    return decode_levels(mode, nlevels, levels, box_astride, box_c0, cls_astride, cls_c0, conf_c0, A, C, B, img_h, img_w,
                         bbox, class_idx, score, N, stream);
}

extern "C" int mydet_decode_uv5_levels_f32(int nlevels, const mydet_decode_level *levels, int box_astride, int box_c0,
                                           int cls_astride, int cls_c0, int conf_c0, int A, int C, int B, int img_h,
                                           int img_w, float *bbox, int64_t *class_idx, float *score, int64_t N,
                                           void *stream) {
    return decode_levels(DECODE_UV5, nlevels, levels, box_astride, box_c0, cls_astride, cls_c0, conf_c0, A, C, B, img_h,
                         img_w, bbox, class_idx, score, N, stream);
}

extern "C" int mydet_decode_f32(int mode, const float *box, int64_t ldbox, int box_astride, int box_c0,
                                const float *cls, int64_t ldcls, int cls_astride, int cls_c0, int conf_c0,
                                const float *anchors_wh, int A, int C, int B, int H, int W, float stride,
                                int img_h, int img_w, float *bbox, int64_t *class_idx, float *score, int64_t N,
                                int64_t n_off, void *stream) {
    mydet_decode_level lv;
    lv.box = box; lv.ldbox = ldbox; lv.cls = cls; lv.ldcls = ldcls; lv.anchors_wh = anchors_wh;
    lv.H = H; lv.W = W; lv.stride = stride; lv.n_off = n_off;
    return mydet_decode_levels_f32(mode, 1, &lv, box_astride, box_c0, cls_astride, cls_c0, conf_c0, A, C, B, img_h,
                                   img_w, bbox, class_idx, score, N, stream);
}
