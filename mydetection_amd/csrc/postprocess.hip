// Batched post-processing: confidence filter -> top-k -> class-aware greedy NMS.
//
// One 1024-thread workgroup per image; the N candidates (25 200 for YOLOv3 @640^2)
// never leave HBM and only <= 512 survivors per image are written.  The work is
// latency-bound (<= 512 boxes, <= 131k IoUs per image), not bandwidth-bound, so the
// design goal is few dependent steps:
//   1. filter: one coalesced sweep of score[N]; passing candidates become unique 64-bit
//      keys (sortable score bits << 32 | ~index) compacted into an HBM scratch strip.
//   2. top-k (only if more than k pass): the k-th largest key is found by 4096-bin histogram rounds over its bits
//      from the top, then bit by bit on the few keys left -- no sort of the N candidates.  Key order = score desc,
//      index asc, which fixes the tie order torch.topk leaves unspecified.
//   3. bitonic sort of the <= 512 selected in LDS by (class asc, score desc, index asc):
//      this is the reference's output order (per-class loop over sorted unique labels,
//      utils/structures.py:158-167, each class in stable score order), and it makes
//      every class a contiguous segment.
//   4. suppression matrix: bit j of row i set iff j > i, same class, (double)IoU > thr --
//      IoU in the exact float32 operation order of torchvision's CPU nms kernel (this file
//      is built with -ffp-contract=off).
//   5. greedy selection as a fixed point: removed <- OR of the rows of the boxes not removed, all 16 waves per
//      round, until nothing changes (the greedy recursion has one solution, so the fixed point is it; real
//      detections settle in a few rounds); inputs that do not settle in 12 rounds take the sequential form
//      (one wave, 64 boxes at a time, dependent chain on the scalar unit).  Rank-by-popcount compaction follows.
// Replaces ImageObjects.post_process / non_max_suppression (utils/structures.py:92-173).
// The kernel is a template on the candidate row width BW: 4 (cxcywh) or 5 (cxcywhd, rotated boxes).  For BW = 5 every step
// above reads columns 0-3 only -- the reference's NMS ignores the angle for 'cxcywhd' (utils/structures.py:137-149) -- and
// the angle is copied with its box into the output rows (5 wide) or into the ANGLE plane of a rotated record.
// The second template parameter ROT (BW = 5 only; opt-in, the mydet_postprocess_*rotnms_f32 entry points) replaces step 4's
// pair test alone: the IoU is the exact area of intersection of the two ROTATED rectangles (rot_iou.h) and a pair is
// suppressed when (double)IoU >= thr -- the `>=` of the reference's nms_rotbb (utils/bbox_ops.py:290).  Every other step
// is shared, so the order, the tie rule and the record layout are those of the <5, false> instance.
// The third template parameter IOS (axis-aligned pair test only; the merge of tile records below) divides the intersection
// by the smaller of the two areas instead of by the union.
// The fourth template parameter MODE (axis-aligned pair test only; the mydet_postprocess_*nms_f32 entry points, include/mydet.h
// "NMS modes") keeps steps 1-3 and replaces what follows them: MODE_GROUPS is steps 4-5 with ONE group of all selected boxes
// (class-agnostic hard NMS), MODE_SOFT is Soft-NMS (no matrix: a wave owns a group, a pick is one wave reduction), MODE_MERGE is
// steps 4-5 and then the score-weighted mean of every kept box's cluster.  All three end in emit_ranked() instead of step 6.
// MODE 0 is the shipped kernel: every `if constexpr (MODE != 0)` below is discarded from it.
#include "common.h"
#include "rot_iou.h"

namespace {

constexpr int KMAX = 512;
constexpr int NT = 1024;
constexpr int IDX_BITS = 20;      // sort key = class (12 bits) | ~score (32) | candidate index (20)
constexpr int CLS_SHIFT = 32 + IDX_BITS;

struct PPArgs {
    const float *bbox;
    const int64_t *cidx;
    const float *score;
    int64_t N;
    float conf;
    double nms;
    int topk;
    int32_t *count;
    float *obox;
    int64_t *ocls;
    float *oscore;
    int32_t *oidx;
    float *oang;                      // BW = 5 only: the angle plane of a rotated record (obox then has 4-float rows), or null
    int64_t oang_st;
    // per-image strides of the five outputs, in elements of each (dense arrays, or fields of one wire record)
    int64_t count_st, obox_st, ocls_st, oscore_st, oidx_st;
    int count_pad;                    // zero words written behind the count (record header padding)
    unsigned long long *scratch;
};

// The kernel argument of the MODE != 0 instances: the shipped instances keep PPArgs as it is
struct PPModeArgs : PPArgs {
    int kind;                         // MYDET_NMS_*
    int agn;                          // one group of all selected boxes
    double sigma;
    float min_score;
};

constexpr int MODE_GROUPS = 1, MODE_SOFT = 2, MODE_MERGE = 3;
template <int MODE> struct ArgsOf { using type = PPModeArgs; };
template <> struct ArgsOf<0> { using type = PPArgs; };

// Order-preserving map of the float32 scores that pass the filter (never a NaN) to unsigned.  -0.0f takes the key of +0.0f:
// the two compare equal, so between them the candidate index decides, as it does for any other tie.
__device__ __forceinline__ unsigned sortable(float f) {
    unsigned u = __float_as_uint(f);
    if (u == 0x80000000u) u = 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// ---- NMS modes (MODE != 0 of the kernel below) ----
// The four helpers here restate lines of the kernel (the pair test of step 4, the sort of step 3, the row stores of step 6)
// for the code the modes add.  The kernel's own lines do not call them: routing the shipped instances through helpers changed
// their register allocation, and they are held to the instruction stream they had (profiles/nms_modes.md).

// The axis-aligned IoU of boxes i and j from their corners and areas, in the float32 operation order of step 4 (torchvision's
// CPU nms kernel).  0/0 (two boxes without area) is NaN.
__device__ __forceinline__ float pair_iou(float ix1, float iy1, float ix2, float iy2, float ia,
                                          float jx1, float jy1, float jx2, float jy2, float ja) {
    const float xx1 = fmaxf(ix1, jx1), yy1 = fmaxf(iy1, jy1);
    const float xx2 = fminf(ix2, jx2), yy2 = fminf(iy2, jy2);
    const float ww = fmaxf(0.0f, xx2 - xx1), hh = fmaxf(0.0f, yy2 - yy1);
    const float inter = ww * hh;
    return inter / (ia + ja - inter);
}

// ascending bitonic sort of KMAX keys in LDS by the first KMAX threads of the workgroup; every thread takes the barriers
__device__ __forceinline__ void bitonic_sort_kmax(unsigned long long *a, int tid) {
    for (int k = 2; k <= KMAX; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            if (tid < KMAX) {
                const int ixj = tid ^ j;
                if (ixj > tid) {
                    const unsigned long long x = a[tid], c = a[ixj];
                    const bool up = (tid & k) == 0;
                    if ((x > c) == up) { a[tid] = c; a[ixj] = x; }
                }
            }
            __syncthreads();
        }
    }
}

// one output row `pos` of image b: box columns 0-3, the angle (BW = 5), class, score and candidate index
template <int BW>
__device__ __forceinline__ void write_row(const PPArgs &p, int b, int pos, f32x4 v, float ang, int64_t cls, float score, unsigned idx) {
    if constexpr (BW == 4) {
        *reinterpret_cast<f32x4 *>(p.obox + b * p.obox_st + pos * 4) = v;
    } else if (p.oang) {                    // rotated record: the 512 x 4 box plane + the angle plane
        *reinterpret_cast<f32x4 *>(p.obox + b * p.obox_st + pos * 4) = v;
        p.oang[b * p.oang_st + pos] = ang;
    } else {
        float *d = p.obox + b * p.obox_st + pos * BW;
        d[0] = v[0]; d[1] = v[1]; d[2] = v[2]; d[3] = v[3]; d[4] = ang;
    }
    p.ocls[b * p.ocls_st + pos] = cls;
    p.oscore[b * p.oscore_st + pos] = score;
    p.oidx[b * p.oidx_st + pos] = (int32_t)idx;
}

// zero rows from `total` to topk, then the count word (and the record header's padding behind it)
template <int BW>
__device__ __forceinline__ void finish_rows(const PPArgs &p, int b, int total, bool bad, int tid) {
    for (int r = total + tid; r < p.topk; r += NT) {
        if constexpr (BW == 4) {
            *reinterpret_cast<f32x4 *>(p.obox + b * p.obox_st + r * 4) = f32x4{0.f, 0.f, 0.f, 0.f};
        } else if (p.oang) {
            *reinterpret_cast<f32x4 *>(p.obox + b * p.obox_st + r * 4) = f32x4{0.f, 0.f, 0.f, 0.f};
            p.oang[b * p.oang_st + r] = 0.f;
        } else {
#pragma unroll
            for (int c = 0; c < BW; ++c) p.obox[b * p.obox_st + r * BW + c] = 0.f;
        }
        p.ocls[b * p.ocls_st + r] = 0;
        p.oscore[b * p.oscore_st + r] = 0.f;
        p.oidx[b * p.oidx_st + r] = 0;
    }
    if (tid <= p.count_pad) p.count[b * p.count_st + tid] = tid == 0 ? (bad ? MYDET_COUNT_BAD_CLASS : total) : 0;
}

// What the modes keep per selected box, in the 32 KiB of the suppression matrix (free in MODE_SOFT, and behind step 5 in the
// other two).  Position = place in the sorted selected list: groups are contiguous there and in order P.
struct ModeLds {
    unsigned long long *okey;         // [KMAX] output order keys
    float *t;                         // [KMAX] the score a box is emitted with (soft kinds: the working score at its pick)
    float *mcx, *mcy, *mw, *mh;       // [KMAX] MODE_MERGE: the merged box
    int *rank;                        // [KMAX] place in the group's selection order, -1 = not emitted
    int *gbeg;                        // [KMAX] first positions of the groups, in any order
    __device__ explicit ModeLds(unsigned long long *base) {
        okey = base;
        t = reinterpret_cast<float *>(base + KMAX);
        mcx = t + KMAX; mcy = mcx + KMAX; mw = mcy + KMAX; mh = mw + KMAX;
        rank = reinterpret_cast<int *>(mh + KMAX);
        gbeg = rank + KMAX;
    }
};
static_assert(KMAX * (8 + 4 * 7) <= KMAX * 8 * 8, "ModeLds fits the suppression matrix");

struct SelLds {                       // the selected list after step 4's first half
    const unsigned long long *key;
    const float *x1, *y1, *x2, *y2, *area;
    const int *cls, *segend;
};

// Soft-NMS (Bodla et al. 2017) of every group; include/mydet.h has the rules.  A wave owns a group: lane l holds its boxes
// l, l + 64, ... (8 for a group of 512) with their working scores in registers.  A pick is a wave maximum over
// (sortable(t), ~candidate index, position) and the decay that follows is 8 pair values per lane, so the 512 dependent picks of
// the longest group need no workgroup barrier.  Writes t and rank of every emitted box.
__device__ void soft_groups(const PPModeArgs &p, const float *sc, const SelLds &s, const ModeLds &m, int ngroups, int tid) {
    constexpr int R = KMAX / 64;
    const int wave = tid >> 6, lane = tid & 63;
    const unsigned min_key = sortable(p.min_score);
    const bool gaussian = p.kind == MYDET_NMS_SOFT_GAUSSIAN;
    for (int g = wave; g < ngroups; g += NT / 64) {
        const int g0 = m.gbeg[g], g1 = s.segend[g0];
        float x1[R], y1[R], x2[R], y2[R], ar[R], t[R];
        unsigned low[R];                                     // (~index) << 9 | position: the tie order, then where the box is
        unsigned alive = 0u;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int pos = g0 + lane + 64 * r;
            x1[r] = y1[r] = x2[r] = y2[r] = ar[r] = t[r] = 0.f;
            low[r] = 0u;
            if (pos < g1) {
                const unsigned idx = (unsigned)(s.key[pos] & ((1ull << IDX_BITS) - 1));
                x1[r] = s.x1[pos]; y1[r] = s.y1[pos]; x2[r] = s.x2[pos]; y2[r] = s.y2[pos]; ar[r] = s.area[pos];
                t[r] = sc[idx];
                low[r] = ((((1u << IDX_BITS) - 1u) - idx) << 9) | (unsigned)pos;
                alive |= 1u << r;
            }
        }
        for (int emitted = 0;; ++emitted) {
            unsigned long long best = 0ull;                  // a live box has a key above 2^60: scores are >= 0 here
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const unsigned long long k = ((unsigned long long)sortable(t[r]) << 29) | low[r];
                if (((alive >> r) & 1u) && k > best) best = k;
            }
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) {
                const unsigned long long o = __shfl_xor(best, off);
                best = o > best ? o : best;
            }
            if (best == 0ull || (unsigned)(best >> 29) < min_key) break;          // uniform: nothing left, or not t >= min_score
            const int wpos = (int)(best & (KMAX - 1));
            const float bx1 = s.x1[wpos], by1 = s.y1[wpos], bx2 = s.x2[wpos], by2 = s.y2[wpos], ba = s.area[wpos];
#pragma unroll
            for (int r = 0; r < R; ++r) {
                if (!((alive >> r) & 1u)) continue;
                if ((int)(low[r] & (KMAX - 1)) == wpos) {
                    m.t[wpos] = t[r];
                    m.rank[wpos] = emitted;
                    alive &= ~(1u << r);
                    continue;
                }
                const float o = pair_iou(bx1, by1, bx2, by2, ba, x1[r], y1[r], x2[r], y2[r], ar[r]);
                if (gaussian) {
                    // o == 0 gives the weight exp(-0) = 1 exactly: skipped; a NaN o leaves t as it is
                    if (o == o && o != 0.0f) t[r] = t[r] * (float)exp(-((double)o * (double)o) / p.sigma);
                } else if ((double)o > p.nms) {
                    t[r] = t[r] * (1.0f - o);
                }
                if (t[r] != t[r]) alive &= ~(1u << r);       // inf * 0: a box without a score is dropped
            }
        }
    }
}

// MODE_MERGE, one lane per kept box i: the score-weighted mean of the corners of i and of every box of its group that i's
// pair value puts above the threshold, accumulated in float64 in ascending position (order P).
__device__ void merge_clusters(const PPModeArgs &p, const SelLds &s, const ModeLds &m, const unsigned long long *removed, int nsel, int tid) {
    if (tid >= nsel || ((removed[tid >> 6] >> (tid & 63)) & 1ull)) return;
    const int ic = s.cls[tid];
    int lo = 0, hi = tid;                                    // first position of my group: lower bound of my class
    if (p.agn) hi = 0;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (s.cls[mid] == ic) hi = mid; else lo = mid + 1;
    }
    const int e = s.segend[tid];
    const float ix1 = s.x1[tid], iy1 = s.y1[tid], ix2 = s.x2[tid], iy2 = s.y2[tid], ia = s.area[tid];
    double W = 0.0, X1 = 0.0, Y1 = 0.0, X2 = 0.0, Y2 = 0.0;
    for (int j = lo; j < e; ++j) {
        const float jx1 = s.x1[j], jy1 = s.y1[j], jx2 = s.x2[j], jy2 = s.y2[j];
        const bool in = j == tid || (double)pair_iou(ix1, iy1, ix2, iy2, ia, jx1, jy1, jx2, jy2, s.area[j]) > p.nms;
        if (in) {
            const double w = (double)m.t[j];
            W += w;
            X1 += w * (double)jx1; Y1 += w * (double)jy1; X2 += w * (double)jx2; Y2 += w * (double)jy2;
        }
    }
    const double x1 = X1 / W, y1 = Y1 / W, x2 = X2 / W, y2 = Y2 / W;
    m.mcx[tid] = (float)((x1 + x2) * 0.5); m.mcy[tid] = (float)((y1 + y2) * 0.5);
    m.mw[tid] = (float)(x2 - x1); m.mh[tid] = (float)(y2 - y1);
}

// The output of every mode: the emitted boxes by (class ascending, rank in the group's selection order), the rest zero.
template <int BW, int MODE>
__device__ void emit_ranked(const PPArgs &p, int b, const float *bb, const int64_t *ci, const SelLds &s, const ModeLds &m,
                            int *s_total, int nsel, bool bad, int tid) {
    if (tid < KMAX)
        m.okey[tid] = tid < nsel && m.rank[tid] >= 0
                          ? ((unsigned long long)s.cls[tid] << 20) | ((unsigned long long)m.rank[tid] << 10) | (unsigned long long)tid
                          : ~0ull;
    if (tid == 0) *s_total = 0;
    __syncthreads();
    bitonic_sort_kmax(m.okey, tid);
    if (tid < KMAX && m.okey[tid] != ~0ull && (tid == KMAX - 1 || m.okey[tid + 1] == ~0ull)) *s_total = tid + 1;
    __syncthreads();
    const int total = bad ? 0 : *s_total;
    if (tid < total) {
        const int pos = (int)(m.okey[tid] & 1023ull);
        const unsigned idx = (unsigned)(s.key[pos] & ((1ull << IDX_BITS) - 1));
        const float *r = bb + (int64_t)idx * BW;
        f32x4 v;
        if constexpr (MODE == MODE_MERGE) v = f32x4{m.mcx[pos], m.mcy[pos], m.mw[pos], m.mh[pos]};
        else if constexpr (BW == 4) v = *reinterpret_cast<const f32x4 *>(r);
        else v = f32x4{r[0], r[1], r[2], r[3]};
        float ang = 0.f;
        if constexpr (BW == 5) ang = r[4];
        write_row<BW>(p, b, tid, v, ang, ci[idx], m.t[pos], idx);
    }
    finish_rows<BW>(p, b, total, bad, tid);
}

template <int BW, bool ROT, bool IOS = false, int MODE = 0>
__global__ __launch_bounds__(NT) void postprocess_kernel(const typename ArgsOf<MODE>::type p) {
    static_assert(!ROT || BW == 5, "the rotated IoU needs the angle column");
    static_assert(!(ROT && IOS), "intersection over smaller is defined for the axis-aligned test only");
    static_assert(MODE == 0 || !ROT, "the NMS modes use the axis-aligned pair value");
    static_assert(MODE != MODE_MERGE || BW == 4, "a mean of angles is not defined");
    __shared__ unsigned long long s_key[KMAX];
    __shared__ unsigned long long s_mask[KMAX * 8];
    // ROT: the seven planes of rotiou::Box -- s_x1, s_y1 = centre, s_x2, s_y2 = hori, s_vx, s_vy = verti, s_area
    __shared__ float s_x1[KMAX], s_y1[KMAX], s_x2[KMAX], s_y2[KMAX], s_area[KMAX];
    __shared__ float s_vx[ROT ? KMAX : 1], s_vy[ROT ? KMAX : 1];
    __shared__ int s_cls[KMAX], s_segend[KMAX];
    __shared__ int s_cnt[3];
    __shared__ unsigned long long s_removed[8];
    __shared__ int s_n, s_nsel, s_bad;

    const int tid = threadIdx.x;
    const int b = blockIdx.x;
    const float *sc = p.score + (int64_t)b * p.N;
    const int64_t *ci = p.cidx + (int64_t)b * p.N;
    const float *bb = p.bbox + (int64_t)b * p.N * BW;
    unsigned long long *keys = p.scratch + (int64_t)b * p.N;
    const int N = (int)p.N;

    if (tid == 0) { s_n = 0; s_nsel = 0; s_bad = 0; }
    __syncthreads();
    // 1. filter (>= in float32, as `self.scores >= conf_thres`)
    //    FU independent loads in flight per thread (a sweep of 76 725 scores -- EfficientDet-D1 -- is five dependent
    //    round trips to memory other XCDs have just written instead of ten); a wave reserves its slots with ONE LDS
    //    atomic (ballot + popcount ranks), so the strip order varies between runs but the key set does not -- and only
    //    the set is used.
    constexpr int FU = 16;
    for (int base = 0; base < N; base += FU * NT) {
        float s8[FU];
#pragma unroll
        for (int u = 0; u < FU; ++u) {
            const int i = base + u * NT + tid;
            s8[u] = __builtin_nontemporal_load(sc + (i < N ? i : N - 1));      // read once; clamped, masked below
        }
#pragma unroll
        for (int u = 0; u < FU; ++u) {
            const int i = base + u * NT + tid;
            const bool pass = i < N && s8[u] >= p.conf;
            const unsigned long long m = __ballot(pass);
            if (m) {                                            // wave-uniform
                int start = 0;
                if ((tid & 63) == 0) start = atomicAdd(&s_n, __popcll(m));
                start = __shfl(start, 0);
                if (pass)
                    keys[start + __popcll(m & ((1ull << (tid & 63)) - 1ull))] =
                        ((unsigned long long)sortable(s8[u]) << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)i);
            }
        }
    }
    __syncthreads();
    const int n = s_n;
    // scratch written above is re-read by other threads of this workgroup only
    __threadfence_block();

    // 2. k-th largest key (only if more than k pass).  4096-bin histogram rounds fix its bits twelve at a time from the
    //    top (one LDS atomic per key that still matches, a block-wide suffix scan finds the bin holding the wanted
    //    rank) until at most 1024 keys share the prefix -- two rounds for distinct scores, up to five when thousands
    //    of candidates tie on one score and only the index bits tell them apart.  Those keys are compacted into LDS
    //    and the remaining bits are built bit by bit on the list (ballot + popcount counting, stops as soon as a
    //    candidate cuts off exactly the wanted number).  The first 16 keys of a thread stay in registers; the others
    //    are re-read with eight loads in flight.
    unsigned long long kth = 0;
    if (n > p.topk) {
        constexpr int RK = 16, LIST = 1024;
        __shared__ int s_wtot[NT / 64], s_sel[3], s_m;
        unsigned *hist = reinterpret_cast<unsigned *>(s_mask);                 // 4096 bins (s_mask is free until step 4)
        unsigned long long *list = s_mask + 2048;                              // LIST keys behind the histogram
        unsigned long long rk[RK];
#pragma unroll
        for (int j = 0; j < RK; ++j) rk[j] = tid + j * NT < n ? keys[tid + j * NT] : 0ull;
        const int wave = tid >> 6, lane = tid & 63;
        // keys beyond the register-resident ones: eight independent loads in flight, then `f` on each
        auto for_tail = [&](auto &&f) {
            for (int base = tid + RK * NT; base < n; base += 8 * NT) {
                unsigned long long kk[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) kk[u] = base + u * NT < n ? keys[base + u * NT] : 0ull;
#pragma unroll
                for (int u = 0; u < 8; ++u)
                    if (base + u * NT < n) f(kk[u]);
            }
        };
        unsigned long long prefix = 0;
        int need = p.topk;                                  // rank of the wanted key among the keys matching `prefix`
        int low = 64;                                       // bits of `prefix` not fixed yet
        for (int level = 0; level < 5; ++level) {
            const int shift = 52 - 12 * level;
            for (int i = tid; i < 4096; i += NT) hist[i] = 0u;
            __syncthreads();
            auto tally = [&](unsigned long long k) {
                if (level == 0 || (k >> low) == (prefix >> low)) atomicAdd(&hist[(unsigned)(k >> shift) & 4095u], 1u);
            };
#pragma unroll
            for (int j = 0; j < RK; ++j)
                if (tid + j * NT < n) tally(rk[j]);
            for_tail(tally);
            __syncthreads();
            // thread t owns bins 4t..4t+3; suffix sums over the threads above it locate the bin of rank `need`
            const unsigned c0 = hist[4 * tid], c1 = hist[4 * tid + 1], c2 = hist[4 * tid + 2], c3 = hist[4 * tid + 3];
            const int own = (int)(c0 + c1 + c2 + c3);
            int suf = own;                                   // inclusive suffix sum inside the wave
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const int v = __shfl_down(suf, off);
                if (lane + off < 64) suf += v;
            }
            if (lane == 0) s_wtot[wave] = suf;
            __syncthreads();
            int above = suf - own;                           // keys in bins above this thread's four
            for (int w = wave + 1; w < NT / 64; ++w) above += s_wtot[w];
            if (above < need && above + own >= need) {       // exactly one thread
                const unsigned c[4] = {c0, c1, c2, c3};
                int a = above, bsel = 0;
#pragma unroll
                for (int q = 3; q >= 0; --q) {
                    if (a < need && a + (int)c[q] >= need) { bsel = q; break; }
                    a += (int)c[q];
                }
                s_sel[0] = 4 * tid + bsel;
                s_sel[1] = a;
                if constexpr (MODE == 0) s_sel[2] = (int)c[bsel];
                else s_sel[2] = (int)(bsel == 3 ? c3 : bsel == 2 ? c2 : bsel == 1 ? c1 : c0);   // c[bsel], kept out of scratch
            }
            __syncthreads();
            prefix |= (unsigned long long)(unsigned)s_sel[0] << shift;
            need -= s_sel[1];
            low = shift;
            const int in_bin = s_sel[2];
            __syncthreads();
            if (in_bin <= LIST) break;                       // uniform; after five rounds low = 4: at most 16 keys match
        }
        // keys sharing the fixed prefix -> LDS list (at most LIST of them)
        if (tid == 0) s_m = 0;
        if (tid < 3) s_cnt[tid] = 0;
        __syncthreads();
        auto collect = [&](unsigned long long k) {
            if ((k >> low) == (prefix >> low)) {
                const int pos = atomicAdd(&s_m, 1);
                list[pos < LIST ? pos : LIST - 1] = k;
            }
        };
#pragma unroll
        for (int j = 0; j < RK; ++j)
            if (tid + j * NT < n) collect(rk[j]);
        for_tail(collect);
        __syncthreads();
        const int m = s_m;
        const unsigned long long lk = tid < m ? list[tid] : 0ull;
        for (int bit = low - 1, it = 0; bit >= 0; --bit, ++it) {
            const unsigned long long cand = prefix | (1ull << bit);
            int c = tid < m && lk >= cand ? 1 : 0;
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) c += __shfl_xor(c, off);
            if (lane == 0) atomicAdd(&s_cnt[it % 3], c);
            if (tid == 0) s_cnt[(it + 1) % 3] = 0;
            __syncthreads();
            const int cnt = s_cnt[it % 3];
            if (cnt >= need) prefix = cand;
            if (cnt == need) break;
        }
        kth = prefix;
        __syncthreads();                                    // s_mask is reused by step 4
    }

    // 3. gather the selected, build (class, ~score, index) keys, sort
    for (int i = tid; i < KMAX; i += NT) s_key[i] = ~0ull;
    __syncthreads();
    for (int base = tid; base < n; base += 8 * NT) {         // eight independent key loads in flight
        unsigned long long kk[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) kk[u] = base + u * NT < n ? keys[base + u * NT] : 0ull;
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const unsigned long long k = kk[u];
            if (base + u * NT < n && k >= kth) {
                const int pos = atomicAdd(&s_nsel, 1);
                const unsigned idx = 0xFFFFFFFFu - (unsigned)(k & 0xFFFFFFFFull);
                const unsigned su = (unsigned)(k >> 32);
                const unsigned long long c = (unsigned long long)ci[idx];       // negative ids wrap to huge values
                if (c > 0xFFFull) s_bad = 1;                                    // the sort key has 12 class bits
                s_key[pos] = ((c & 0xFFFull) << CLS_SHIFT) | ((unsigned long long)(~su) << IDX_BITS) | (unsigned long long)idx;
                if constexpr (MODE != 0) {                                      // one group: order P over all selected, no class bits
                    if (p.agn) s_key[pos] = ((unsigned long long)(~su) << IDX_BITS) | (unsigned long long)idx;
                }
            }
        }
    }
    __syncthreads();
    const int nsel = s_nsel;
    const bool bad = s_bad != 0;       // a selected candidate's class id is outside [0, 4096): fail the image loudly
    for (int k = 2; k <= KMAX; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            if (tid < KMAX) {
                const int ixj = tid ^ j;
                if (ixj > tid) {
                    const unsigned long long a = s_key[tid], c = s_key[ixj];
                    const bool up = (tid & k) == 0;
                    if ((a > c) == up) { s_key[tid] = c; s_key[ixj] = a; }
                }
            }
            __syncthreads();
        }
    }

    // 4. corners + areas, then the suppression matrix
    if (tid < nsel) {
        const unsigned long long k = s_key[tid];
        const unsigned idx = (unsigned)(k & ((1ull << IDX_BITS) - 1));
        if constexpr (ROT) {
            const float *r = bb + (int64_t)idx * BW;
            const rotiou::Box q = rotiou::make_box(r[0], r[1], r[2], r[3], r[4]);
            s_x1[tid] = q.cx; s_y1[tid] = q.cy; s_x2[tid] = q.hx; s_y2[tid] = q.hy; s_vx[tid] = q.vx; s_vy[tid] = q.vy;
            s_area[tid] = q.area;
        } else {
            f32x4 v;
            if constexpr (BW == 4) {
                v = *reinterpret_cast<const f32x4 *>(bb + (int64_t)idx * 4);
            } else {                                    // 20-byte rows: columns 0-3, the angle is not used here
                const float *r = bb + (int64_t)idx * BW;
                v = f32x4{r[0], r[1], r[2], r[3]};
            }
            const float hw = v[2] / 2.0f, hh = v[3] / 2.0f;
            const float x1 = v[0] - hw, y1 = v[1] - hh, x2 = v[0] + hw, y2 = v[1] + hh;
            s_x1[tid] = x1; s_y1[tid] = y1; s_x2[tid] = x2; s_y2[tid] = y2;
            s_area[tid] = (x2 - x1) * (y2 - y1);
        }
        s_cls[tid] = (int)(k >> CLS_SHIFT);
        if constexpr (MODE != 0) { if (p.agn) s_cls[tid] = (int)(ci[idx] & 0xFFF); }      // the key holds no class then
    }
    __syncthreads();
    // rows are zero except inside the row's own class segment (classes are contiguous after the sort).  
    for (int w = tid; w < nsel * 8; w += NT) s_mask[w] = 0ull;
    if (tid < nsel) {                                   // end of my class segment: upper bound of my class
        const int ic = s_cls[tid];
        int lo = tid + 1, hi = nsel;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (s_cls[mid] == ic) lo = mid + 1; else hi = mid;
        }
        if constexpr (MODE != 0) { if (p.agn) lo = nsel; }
        s_segend[tid] = lo;
    }
    __syncthreads();
    if constexpr (MODE == MODE_SOFT) {
        __shared__ int s_ng;
        const SelLds sel{s_key, s_x1, s_y1, s_x2, s_y2, s_area, s_cls, s_segend};
        const ModeLds m(s_mask);
        if (tid == 0) s_ng = 0;
        __syncthreads();                                    // and the zeroing of s_mask above is done
        if (tid < nsel) {
            m.rank[tid] = -1;
            if (tid == 0 || (!p.agn && s_cls[tid - 1] != s_cls[tid])) m.gbeg[atomicAdd(&s_ng, 1)] = tid;
        }
        __syncthreads();
        soft_groups(p, sc, sel, m, s_ng, tid);
        __syncthreads();
        emit_ranked<BW, MODE>(p, b, bb, ci, sel, m, &s_cnt[0], nsel, bad, tid);
        return;
    }
    // a wave owns rows i = wave, wave+16, ...; for each it walks only the 64-box words that overlap
    // [i+1, end of i's class segment): lane = one j, the word is the wave's ballot (no atomics, conflict-free LDS)
    {
        const int wave = tid >> 6, lane = tid & 63;
        for (int i = wave; i < nsel; i += NT / 64) {
            const int e = s_segend[i];
            const float ix1 = s_x1[i], iy1 = s_y1[i], ix2 = s_x2[i], iy2 = s_y2[i], ia = s_area[i];
            for (int w = (i + 1) >> 6; w * 64 < e; ++w) {
                const int j = w * 64 + lane;
                bool sup = false;
                if constexpr (ROT) {
                    if (j > i && j < e) {
                        const rotiou::Box bi{ix1, iy1, ix2, iy2, s_vx[i], s_vy[i], ia};
                        const rotiou::Box bj{s_x1[j], s_y1[j], s_x2[j], s_y2[j], s_vx[j], s_vy[j], s_area[j]};
                        sup = (double)rotiou::rot_iou(bi, bj) >= p.nms;          // NaN (both areas 0): not suppressed
                    }
                } else if (j > i && j < e) {
                    const float xx1 = fmaxf(ix1, s_x1[j]), yy1 = fmaxf(iy1, s_y1[j]);
                    const float xx2 = fminf(ix2, s_x2[j]), yy2 = fminf(iy2, s_y2[j]);
                    const float ww = fmaxf(0.0f, xx2 - xx1), hh = fmaxf(0.0f, yy2 - yy1);
                    const float inter = ww * hh;
                    float ovr;
                    if constexpr (IOS) ovr = inter / fminf(ia, s_area[j]);       // 0/0 (two boxes without area): NaN, not suppressed
                    else ovr = inter / (ia + s_area[j] - inter);
                    sup = (double)ovr > p.nms;
                }
                const unsigned long long bits = __ballot(sup);
                if (lane == 0) s_mask[i * 8 + w] = bits;
            }
        }
    }
    __syncthreads();

    // 5. greedy selection.  kept[i] = no kept j < i suppresses i, and that recursion has exactly one solution, so
    //    any fixed point of  removed <- OR of the rows of the boxes not in removed  IS the greedy result.  Starting
    //    from removed = 0, round t fixes every box whose chain of (suppressor of suppressor of ...) is shorter than
    //    t -- a handful of rounds on real detections -- and each round is one parallel OR-reduction of the 512 x 8
    //    mask words by all 16 waves.  Inputs that have not settled after MAX_ROUNDS fall back to the sequential scan.
    constexpr int MAX_ROUNDS = 12;
    __shared__ unsigned long long s_part[NT / 64][8];
    __shared__ int s_changed;
    bool settled = false;
    {
        const int wave = tid >> 6, lane = tid & 63;
        // rows r = tid and tid + 512 (two half-rows per thread would not balance; a thread owns 4 words of a row)
        const int row = tid >> 1, w0 = (tid & 1) * 4;
        unsigned long long mine[4];
#pragma unroll
        for (int w = 0; w < 4; ++w) mine[w] = row < nsel ? s_mask[row * 8 + w0 + w] : 0ull;
        if (tid < 8) s_removed[tid] = 0ull;
        __syncthreads();
        for (int round = 0; round < MAX_ROUNDS; ++round) {
            const bool kept = row < nsel && !((s_removed[row >> 6] >> (row & 63)) & 1ull);
            unsigned long long acc[4];
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                unsigned lo = kept ? (unsigned)mine[w] : 0u, hi = kept ? (unsigned)(mine[w] >> 32) : 0u;
                // lanes with the same parity hold the same four words: reduce over stride-2 partners
#pragma unroll
                for (int off = 32; off >= 2; off >>= 1) {
                    lo |= __shfl_xor(lo, off);
                    hi |= __shfl_xor(hi, off);
                }
                acc[w] = ((unsigned long long)hi << 32) | lo;
            }
            if (lane < 2) {
#pragma unroll
                for (int w = 0; w < 4; ++w) s_part[wave][lane * 4 + w] = acc[w];
            }
            if (tid == 0) s_changed = 0;
            __syncthreads();
            if (tid < 8) {
                unsigned long long r = 0ull;
#pragma unroll
                for (int v = 0; v < NT / 64; ++v) r |= s_part[v][tid];
                if (r != s_removed[tid]) { s_removed[tid] = r; s_changed = 1; }
            }
            __syncthreads();
            if (!s_changed) { settled = true; break; }         // uniform: read after the barrier by every thread
            __syncthreads();                                    // s_changed is reset at the top of the next round
        }
    }
    // sequential form (wave 0; lane w < 8 owns word w of the removed set): one wave, 64 boxes at a time.  Lane l
    // holds row 64c+l.  Inside a chunk the dependent chain runs on the scalar unit only (bit test on a 64-bit scalar,
    // v_readlane of the diagonal word, scalar OR); the chunk's survivors then OR their rows into the later words.
    if (!settled && tid < 64) {
        const int lane = tid;
        unsigned long long removed[8];
#pragma unroll
        for (int w = 0; w < 8; ++w) removed[w] = 0ull;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            if (c * 64 < nsel) {                                   // uniform
                const int r = c * 64 + lane;
                const bool valid = r < nsel;
                unsigned long long mw[8];
#pragma unroll
                for (int w = c; w < 8; ++w) mw[w] = valid ? s_mask[r * 8 + w] : 0ull;
                const unsigned dlo = (unsigned)mw[c], dhi = (unsigned)(mw[c] >> 32);
                unsigned long long rc = removed[c];
                const int nb = nsel - c * 64 < 64 ? nsel - c * 64 : 64;
                for (int bq = 0; bq < nb; ++bq) {
                    const unsigned long long d = ((unsigned long long)(unsigned)__builtin_amdgcn_readlane(dhi, bq) << 32) |
                                                 (unsigned long long)(unsigned)__builtin_amdgcn_readlane(dlo, bq);
                    if (!((rc >> bq) & 1ull)) rc |= d;
                }
                removed[c] = rc;
                const bool kept = valid && !((rc >> lane) & 1ull);
#pragma unroll
                for (int w = c + 1; w < 8; ++w) {
                    unsigned lo = kept ? (unsigned)mw[w] : 0u, hi = kept ? (unsigned)(mw[w] >> 32) : 0u;
#pragma unroll
                    for (int off = 32; off >= 1; off >>= 1) {
                        lo |= __shfl_xor(lo, off);
                        hi |= __shfl_xor(hi, off);
                    }
                    removed[w] |= ((unsigned long long)hi << 32) | lo;
                }
            }
        }
#pragma unroll
        for (int w = 0; w < 8; ++w)
            if (lane == w) s_removed[w] = removed[w];
    }
    __syncthreads();
    if constexpr (MODE != 0) {                              // s_mask is free: the greedy result is s_removed
        const SelLds sel{s_key, s_x1, s_y1, s_x2, s_y2, s_area, s_cls, s_segend};
        const ModeLds m(s_mask);
        if (tid < nsel) {
            const unsigned idx = (unsigned)(s_key[tid] & ((1ull << IDX_BITS) - 1));
            m.t[tid] = sc[idx];
            m.rank[tid] = ((s_removed[tid >> 6] >> (tid & 63)) & 1ull) ? -1 : tid;
        }
        __syncthreads();
        if constexpr (MODE == MODE_MERGE) {
            merge_clusters(p, sel, m, s_removed, nsel, tid);
            __syncthreads();
        }
        emit_ranked<BW, MODE>(p, b, bb, ci, sel, m, &s_cnt[0], nsel, bad, tid);
        return;
    }

    // 6. survivors, ranked by popcount, in sorted (class asc, score desc) order
    int total = 0;
    {
        int before = 0;
        const int myw = tid >> 6;
        for (int w = 0; w < 8; ++w) {
            const int lim = nsel - w * 64;
            unsigned long long valid = lim >= 64 ? ~0ull : (lim <= 0 ? 0ull : ((1ull << lim) - 1ull));
            const unsigned long long kept = ~s_removed[w] & valid;
            const int pc = __popcll(kept);
            if (w < myw) before += pc;
            total += pc;
        }
        if (bad) total = 0;
        if (tid < nsel && !bad) {
            const unsigned long long kept = ~s_removed[myw];
            if ((kept >> (tid & 63)) & 1ull) {
                const int pos = before + __popcll(kept & ((1ull << (tid & 63)) - 1ull));
                const unsigned long long k = s_key[tid];
                const unsigned idx = (unsigned)(k & ((1ull << IDX_BITS) - 1));
                if constexpr (BW == 4) {
                    *reinterpret_cast<f32x4 *>(p.obox + b * p.obox_st + pos * 4) = *reinterpret_cast<const f32x4 *>(bb + (int64_t)idx * 4);
                } else {
                    const float *r = bb + (int64_t)idx * BW;
                    if (p.oang) {                       // rotated record: the 512 x 4 box plane + the angle plane
                        *reinterpret_cast<f32x4 *>(p.obox + b * p.obox_st + pos * 4) = f32x4{r[0], r[1], r[2], r[3]};
                        p.oang[b * p.oang_st + pos] = r[4];
                    } else {
                        float *d = p.obox + b * p.obox_st + pos * BW;
#pragma unroll
                        for (int c = 0; c < BW; ++c) d[c] = r[c];
                    }
                }
                p.ocls[b * p.ocls_st + pos] = ci[idx];
                p.oscore[b * p.oscore_st + pos] = sc[idx];
                p.oidx[b * p.oidx_st + pos] = (int32_t)idx;
            }
        }
    }
    for (int r = total + tid; r < p.topk; r += NT) {
        if constexpr (BW == 4) {
            *reinterpret_cast<f32x4 *>(p.obox + b * p.obox_st + r * 4) = f32x4{0.f, 0.f, 0.f, 0.f};
        } else if (p.oang) {
            *reinterpret_cast<f32x4 *>(p.obox + b * p.obox_st + r * 4) = f32x4{0.f, 0.f, 0.f, 0.f};
            p.oang[b * p.oang_st + r] = 0.f;
        } else {
#pragma unroll
            for (int c = 0; c < BW; ++c) p.obox[b * p.obox_st + r * BW + c] = 0.f;
        }
        p.ocls[b * p.ocls_st + r] = 0;
        p.oscore[b * p.oscore_st + r] = 0.f;
        p.oidx[b * p.oidx_st + r] = 0;
    }
    if (tid <= p.count_pad) p.count[b * p.count_st + tid] = tid == 0 ? (bad ? MYDET_COUNT_BAD_CLASS : total) : 0;
}

}  // namespace

// the fields of a wire record (MYDET_REC_*; rot: the rotated record with its angle plane) as the outputs of the kernel
static void record_outputs(PPArgs &p, int32_t *records, bool rot) {
    const int64_t words = rot ? MYDET_REC_ROT_WORDS : MYDET_REC_WORDS;
    p.count = records + MYDET_REC_COUNT;
    p.obox = reinterpret_cast<float *>(records + MYDET_REC_BBOX);
    p.oscore = reinterpret_cast<float *>(records + MYDET_REC_SCORE);
    p.ocls = reinterpret_cast<int64_t *>(records + MYDET_REC_CLASS);
    p.oidx = records + MYDET_REC_INDEX;
    p.oang = rot ? reinterpret_cast<float *>(records + MYDET_REC_ANGLE) : nullptr;
    p.count_pad = MYDET_REC_BBOX - 1; p.count_st = words; p.obox_st = words; p.oscore_st = words;
    p.ocls_st = words / 2; p.oidx_st = words; p.oang_st = rot ? words : 0;
}

template <int BW, bool ROT = false, bool IOS = false, int MODE = 0>
static int launch_postprocess(typename ArgsOf<MODE>::type &p, const float *bbox, const int64_t *class_idx, const float *score, int B, int64_t N,
                              float conf_thres, double nms_thres, int topk, void *scratch, void *stream) {
    if (B <= 0 || N < 0 || topk <= 0 || topk > KMAX) return MYDET_E_BADARG;
    if (N >= (1ll << IDX_BITS)) return MYDET_E_UNSUPP;
    if (!p.count || !p.obox || !p.ocls || !p.oscore || !p.oidx) return MYDET_E_BADARG;
    if (N > 0 && (!bbox || !class_idx || !score || !scratch)) return MYDET_E_BADARG;
    if (((uintptr_t)bbox & 15) || ((uintptr_t)p.obox & 15) || ((uintptr_t)scratch & 7) || ((uintptr_t)p.ocls & 7)) return MYDET_E_BADARG;
    p.bbox = bbox; p.cidx = class_idx; p.score = score; p.N = N; p.conf = conf_thres; p.nms = nms_thres;
    p.topk = topk; p.scratch = (unsigned long long *)scratch;
    hipLaunchKernelGGL((postprocess_kernel<BW, ROT, IOS, MODE>), dim3(B), dim3(NT), 0, (hipStream_t)stream, p);
    return mydet_launch_status();
}

extern "C" int mydet_postprocess_f32(const float *bbox, const int64_t *class_idx, const float *score, int B,
                                     int64_t N, float conf_thres, double nms_thres, int topk, int32_t *count,
                                     float *out_bbox, int64_t *out_class, float *out_score, int32_t *out_index,
                                     void *scratch, void *stream) {
    PPArgs p;
    p.count = count; p.obox = out_bbox; p.ocls = out_class; p.oscore = out_score; p.oidx = out_index;
    p.oang = nullptr; p.oang_st = 0;
    p.count_pad = 0; p.count_st = 1; p.obox_st = (int64_t)topk * 4; p.ocls_st = topk; p.oscore_st = topk; p.oidx_st = topk;
    return launch_postprocess<4>(p, bbox, class_idx, score, B, N, conf_thres, nms_thres, topk, scratch, stream);
}

extern "C" int mydet_postprocess_records_f32(const float *bbox, const int64_t *class_idx, const float *score, int B,
                                             int64_t N, float conf_thres, double nms_thres, int32_t *records,
                                             void *scratch, void *stream) {
    if ((uintptr_t)records & 15) return MYDET_E_BADARG;
    PPArgs p;
    p.oang = nullptr; p.oang_st = 0;
    if (!records) { p.count = nullptr; p.obox = nullptr; p.ocls = nullptr; p.oscore = nullptr; p.oidx = nullptr;
                    return launch_postprocess<4>(p, bbox, class_idx, score, B, N, conf_thres, nms_thres, MYDET_REC_TOPK, scratch, stream); }
    record_outputs(p, records, false);
    return launch_postprocess<4>(p, bbox, class_idx, score, B, N, conf_thres, nms_thres, MYDET_REC_TOPK, scratch, stream);
}

extern "C" int mydet_postprocess_rot_f32(const float *bbox, const int64_t *class_idx, const float *score, int B,
                                         int64_t N, float conf_thres, double nms_thres, int topk, int32_t *count,
                                         float *out_bbox, int64_t *out_class, float *out_score, int32_t *out_index,
                                         void *scratch, void *stream) {
    PPArgs p;
    p.count = count; p.obox = out_bbox; p.ocls = out_class; p.oscore = out_score; p.oidx = out_index;
    p.oang = nullptr; p.oang_st = 0;
    p.count_pad = 0; p.count_st = 1; p.obox_st = (int64_t)topk * 5; p.ocls_st = topk; p.oscore_st = topk; p.oidx_st = topk;
    return launch_postprocess<5>(p, bbox, class_idx, score, B, N, conf_thres, nms_thres, topk, scratch, stream);
}

extern "C" int mydet_postprocess_records_rot_f32(const float *bbox, const int64_t *class_idx, const float *score, int B,
                                                 int64_t N, float conf_thres, double nms_thres, int32_t *records,
                                                 void *scratch, void *stream) {
    if (!records || ((uintptr_t)records & 15)) return MYDET_E_BADARG;
    PPArgs p;
    record_outputs(p, records, true);
    return launch_postprocess<5>(p, bbox, class_idx, score, B, N, conf_thres, nms_thres, MYDET_REC_TOPK, scratch, stream);
}

// The rotated-IoU forms of the two entry points above: arguments, checks and outputs are theirs, the pair test of the NMS
// is rotiou::rot_iou with `>=` (include/mydet.h).
extern "C" int mydet_postprocess_rotnms_f32(const float *bbox, const int64_t *class_idx, const float *score, int B,
                                            int64_t N, float conf_thres, double nms_thres, int topk, int32_t *count,
                                            float *out_bbox, int64_t *out_class, float *out_score, int32_t *out_index,
                                            void *scratch, void *stream) {
    PPArgs p;
    p.count = count; p.obox = out_bbox; p.ocls = out_class; p.oscore = out_score; p.oidx = out_index;
    p.oang = nullptr; p.oang_st = 0;
    p.count_pad = 0; p.count_st = 1; p.obox_st = (int64_t)topk * 5; p.ocls_st = topk; p.oscore_st = topk; p.oidx_st = topk;
    return launch_postprocess<5, true>(p, bbox, class_idx, score, B, N, conf_thres, nms_thres, topk, scratch, stream);
}

extern "C" int mydet_postprocess_records_rotnms_f32(const float *bbox, const int64_t *class_idx, const float *score, int B,
                                                    int64_t N, float conf_thres, double nms_thres, int32_t *records,
                                                    void *scratch, void *stream) {
    if (!records || ((uintptr_t)records & 15)) return MYDET_E_BADARG;
    PPArgs p;
    record_outputs(p, records, true);
    return launch_postprocess<5, true>(p, bbox, class_idx, score, B, N, conf_thres, nms_thres, MYDET_REC_TOPK, scratch, stream);
}

// ---- NMS modes (include/mydet.h): the four entry points above with a mydet_nms_mode ----
// The argument rules of a mode, before any launch.  HARD without `agnostic` is the shipped instance itself.
static int check_mode(const mydet_nms_mode *m, int box_width, float conf_thres) {
    if (!m || m->kind < MYDET_NMS_HARD || m->kind > MYDET_NMS_MERGE || (m->agnostic != 0 && m->agnostic != 1)) return MYDET_E_BADARG;
    if (m->kind == MYDET_NMS_SOFT_LINEAR || m->kind == MYDET_NMS_SOFT_GAUSSIAN) {
        if (!(conf_thres >= 0.0f) || !(m->min_score >= 0.0f)) return MYDET_E_BADARG;
        if (m->kind == MYDET_NMS_SOFT_GAUSSIAN && !(m->sigma > 0.0)) return MYDET_E_BADARG;
    }
    if (m->kind == MYDET_NMS_MERGE) {
        if (!(conf_thres > 0.0f)) return MYDET_E_BADARG;
        if (box_width != 4) return MYDET_E_UNSUPP;
    }
    return 0;
}

template <int BW>
static int launch_mode(PPModeArgs &p, const mydet_nms_mode *m, const float *bbox, const int64_t *class_idx, const float *score, int B,
                       int64_t N, float conf_thres, double nms_thres, int topk, void *scratch, void *stream) {
    const int st = check_mode(m, BW, conf_thres);
    if (st) return st;
    p.kind = m->kind; p.agn = m->agnostic; p.sigma = m->sigma; p.min_score = m->min_score;
    if (m->kind == MYDET_NMS_HARD)
        return m->agnostic ? launch_postprocess<BW, false, false, MODE_GROUPS>(p, bbox, class_idx, score, B, N, conf_thres, nms_thres, topk, scratch, stream)
                           : launch_postprocess<BW>(p, bbox, class_idx, score, B, N, conf_thres, nms_thres, topk, scratch, stream);
    if constexpr (BW == 4) {
        if (m->kind == MYDET_NMS_MERGE)
            return launch_postprocess<4, false, false, MODE_MERGE>(p, bbox, class_idx, score, B, N, conf_thres, nms_thres, topk, scratch, stream);
    }
    return launch_postprocess<BW, false, false, MODE_SOFT>(p, bbox, class_idx, score, B, N, conf_thres, nms_thres, topk, scratch, stream);
}

static void dense_outputs(PPArgs &p, int box_width, int topk, int32_t *count, float *out_bbox, int64_t *out_class, float *out_score,
                          int32_t *out_index) {
    p.count = count; p.obox = out_bbox; p.ocls = out_class; p.oscore = out_score; p.oidx = out_index;
    p.oang = nullptr; p.oang_st = 0;
    p.count_pad = 0; p.count_st = 1; p.obox_st = (int64_t)topk * box_width; p.ocls_st = topk; p.oscore_st = topk; p.oidx_st = topk;
}

extern "C" int mydet_postprocess_nms_f32(const float *bbox, const int64_t *class_idx, const float *score, int B, int64_t N,
                                         float conf_thres, double nms_thres, int topk, const mydet_nms_mode *mode, int32_t *count,
                                         float *out_bbox, int64_t *out_class, float *out_score, int32_t *out_index,
                                         void *scratch, void *stream) {
    PPModeArgs p;
    dense_outputs(p, 4, topk, count, out_bbox, out_class, out_score, out_index);
    return launch_mode<4>(p, mode, bbox, class_idx, score, B, N, conf_thres, nms_thres, topk, scratch, stream);
}

extern "C" int mydet_postprocess_rot_nms_f32(const float *bbox, const int64_t *class_idx, const float *score, int B, int64_t N,
                                             float conf_thres, double nms_thres, int topk, const mydet_nms_mode *mode, int32_t *count,
                                             float *out_bbox, int64_t *out_class, float *out_score, int32_t *out_index,
                                             void *scratch, void *stream) {
    PPModeArgs p;
    dense_outputs(p, 5, topk, count, out_bbox, out_class, out_score, out_index);
    return launch_mode<5>(p, mode, bbox, class_idx, score, B, N, conf_thres, nms_thres, topk, scratch, stream);
}

extern "C" int mydet_postprocess_records_nms_f32(const float *bbox, const int64_t *class_idx, const float *score, int B, int64_t N,
                                                 float conf_thres, double nms_thres, const mydet_nms_mode *mode, int32_t *records,
                                                 void *scratch, void *stream) {
    if (!records || ((uintptr_t)records & 15)) return MYDET_E_BADARG;
    PPModeArgs p;
    record_outputs(p, records, false);
    return launch_mode<4>(p, mode, bbox, class_idx, score, B, N, conf_thres, nms_thres, MYDET_REC_TOPK, scratch, stream);
}

extern "C" int mydet_postprocess_records_rot_nms_f32(const float *bbox, const int64_t *class_idx, const float *score, int B,
                                                     int64_t N, float conf_thres, double nms_thres, const mydet_nms_mode *mode,
                                                     int32_t *records, void *scratch, void *stream) {
    if (!records || ((uintptr_t)records & 15)) return MYDET_E_BADARG;
    PPModeArgs p;
    record_outputs(p, records, true);
    return launch_mode<5>(p, mode, bbox, class_idx, score, B, N, conf_thres, nms_thres, MYDET_REC_TOPK, scratch, stream);
}

// ---- merge of tile records (tiled detection on large frames; include/mydet.h) ----
// The detections of T windows of a frame, already in window pixel coordinates, become the candidates of ONE more run of the
// kernel above: a gather launch writes the B x T*512 candidate arrays into scratch (box centres shifted by the window origin),
// then postprocess_kernel runs on them with conf = -inf.  Nothing of the selection or the NMS is restated here.
namespace {

struct MergeArgs {
    const int32_t *rec;               // record of tile t of frame b at rec + t*tile_st + b*frame_st (words)
    int64_t tile_st, frame_st;
    const int32_t *origins;           // [T][2] = (x0, y0)
    int T;
    float *bbox;                      // [B][T*512][BW]
    int64_t *cidx;                    // [B][T*512]
    float *score;                     // [B][T*512]
    // VIEW instances (fusion of view records below): no origins; window t is view t, mirrored by bits 2t, 2t+1 of `flips`
    unsigned flips;
    float frame_w, frame_h;
    int zero_origin;                  // add the (float)0 origin of a merge with zero origins: -0 becomes +0, as there
};

// One thread per candidate slot (b = blockIdx.y, t*512 + k = blockIdx.x * 256 + tid): lane k reads the 16-byte box row k of
// the tile's box plane and writes the 16-byte candidate row k -- 1 KiB per wave instruction either way.  Slots past the
// tile's count get a NaN score (it fails `>=` against every threshold), box 0 and class 0, so every word of the candidate
// arrays is defined.  A tile whose count is the bad-class sentinel plants ONE candidate with score +inf and class -1 in its
// slot 0: it is among the top 512 whatever else the frame holds, and the kernel above then fails the frame the way it fails
// any image with such a class (count = MYDET_COUNT_BAD_CLASS, zero rows).
// VIEW: the candidates of mydet_fuse_view_records_f32 -- instead of the origin shift, the box is brought back from its
// mirrored view: cx' = frame_w - cx (HFLIP), cy' = frame_h - cy (VFLIP), angle' = -angle when exactly one bit is set.
template <int BW, bool VIEW = false>
__global__ __launch_bounds__(256) void merge_gather_kernel(const MergeArgs a) {
    const int i = blockIdx.x * 256 + threadIdx.x;          // grid.x * 256 == T * 512 exactly
    const int t = i >> 9, k = i & (KMAX - 1);
    const int b = blockIdx.y;
    const int32_t *r = a.rec + (int64_t)t * a.tile_st + (int64_t)b * a.frame_st;
    const int count = r[MYDET_REC_COUNT];
    const int64_t o = (int64_t)b * a.T * KMAX + i;
    f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
    float ang = 0.f, sc = __uint_as_float(0x7FC00000u);
    int64_t c = 0;
    if (count < 0) {
        if (k == 0) { sc = __uint_as_float(0x7F800000u); c = -1; }
    } else if (k < count) {                                // a count above 512 cannot come from the kernel above; k < 512 anyway
        v = *reinterpret_cast<const f32x4 *>(r + MYDET_REC_BBOX + 4 * k);
        if constexpr (BW == 5) ang = reinterpret_cast<const float *>(r + MYDET_REC_ANGLE)[k];
        if constexpr (VIEW) {
            const unsigned f = (a.flips >> (2 * t)) & 3u;
            if (f & MYDET_VIEW_HFLIP) v[0] = a.frame_w - v[0];
            if (f & MYDET_VIEW_VFLIP) v[1] = a.frame_h - v[1];
            if (f == MYDET_VIEW_HFLIP || f == MYDET_VIEW_VFLIP) ang = -ang;
            if (a.zero_origin) { v[0] = v[0] + 0.0f; v[1] = v[1] + 0.0f; }
        } else {
            v[0] = v[0] + (float)a.origins[2 * t];
            v[1] = v[1] + (float)a.origins[2 * t + 1];
        }
        sc = reinterpret_cast<const float *>(r + MYDET_REC_SCORE)[k];
        c = reinterpret_cast<const int64_t *>(r + MYDET_REC_CLASS)[k];
    }
    if constexpr (BW == 4) {
        *reinterpret_cast<f32x4 *>(a.bbox + o * 4) = v;
    } else {                                               // 20-byte rows are not 16-byte aligned: five dword stores
        float *d = a.bbox + o * 5;
        d[0] = v[0]; d[1] = v[1]; d[2] = v[2]; d[3] = v[3]; d[4] = ang;
    }
    a.cidx[o] = c;
    a.score[o] = sc;
}

}  // namespace

// candidate arrays + the key strip of postprocess_kernel: per candidate BW floats, an int64 class, a float score, an 8-byte key
// (every part a multiple of 16 bytes: B * T * 512 candidates)
extern "C" int64_t mydet_merge_tile_records_scratch_bytes(int B, int T, int box_width) {
    if (B <= 0 || T < 1 || T > MYDET_TILES_MAX || (box_width != 4 && box_width != 5)) return 0;
    return (int64_t)B * T * KMAX * (4 * box_width + 8 + 4 + 8);
}

// The argument rules the merge and the fusion of view records share (T windows or views, at most `tmax`); `src` is the
// origins (device) or the flips (host)
static int merge_check_args(const int32_t *tile_records, int64_t tile_stride_words, int64_t frame_stride_words, int B, int T, int tmax,
                            int box_width, const void *src, int metric, int rotated_nms, int agnostic, const int32_t *records,
                            const void *scratch) {
    if (agnostic != 0 && agnostic != 1) return MYDET_E_BADARG;
    if (B <= 0 || T < 1 || T > tmax) return MYDET_E_BADARG;
    if (box_width != 4 && box_width != 5) return MYDET_E_BADARG;
    if (metric != MYDET_MERGE_IOU && metric != MYDET_MERGE_IOS) return MYDET_E_BADARG;
    if (rotated_nms && box_width != 5) return MYDET_E_BADARG;
    if (!tile_records || !src || !records || !scratch) return MYDET_E_BADARG;
    // a record is read with 16-byte loads: the base and both strides keep that alignment
    if (((uintptr_t)tile_records & 15) || ((uintptr_t)records & 15) || ((uintptr_t)scratch & 15) || ((uintptr_t)src & 3)) return MYDET_E_BADARG;
    if (tile_stride_words < 0 || frame_stride_words < 0 || (tile_stride_words & 3) || (frame_stride_words & 3)) return MYDET_E_BADARG;
    return 0;
}

// The candidate arrays in `scratch`; returns what follows them (the key strip of postprocess_kernel)
static void *merge_layout(MergeArgs &a, void *scratch, int64_t BN, int box_width) {
    a.bbox = reinterpret_cast<float *>(scratch);
    a.cidx = reinterpret_cast<int64_t *>(a.bbox + BN * box_width);
    a.score = reinterpret_cast<float *>(a.cidx + BN);
    return a.score + BN;
}

// The second launch of the merge: postprocess_kernel on the gathered candidates with conf = -inf
static int merge_nms(const MergeArgs &a, int B, int64_t N, int box_width, double nms_thres, int metric, int rotated_nms, int agnostic,
                     int32_t *records, void *keys, void *stream) {
    PPModeArgs p;
    record_outputs(p, records, box_width == 5);
    const float conf = -__builtin_inff();
    if (agnostic) {
        p.kind = MYDET_NMS_HARD; p.agn = 1; p.sigma = 0.0; p.min_score = 0.f;
        if (box_width == 4)
            return metric == MYDET_MERGE_IOS
                       ? launch_postprocess<4, false, true, MODE_GROUPS>(p, a.bbox, a.cidx, a.score, B, N, conf, nms_thres, MYDET_REC_TOPK, keys, stream)
                       : launch_postprocess<4, false, false, MODE_GROUPS>(p, a.bbox, a.cidx, a.score, B, N, conf, nms_thres, MYDET_REC_TOPK, keys, stream);
        return metric == MYDET_MERGE_IOS
                   ? launch_postprocess<5, false, true, MODE_GROUPS>(p, a.bbox, a.cidx, a.score, B, N, conf, nms_thres, MYDET_REC_TOPK, keys, stream)
                   : launch_postprocess<5, false, false, MODE_GROUPS>(p, a.bbox, a.cidx, a.score, B, N, conf, nms_thres, MYDET_REC_TOPK, keys, stream);
    }
    if (box_width == 4)
        return metric == MYDET_MERGE_IOS
                   ? launch_postprocess<4, false, true>(p, a.bbox, a.cidx, a.score, B, N, conf, nms_thres, MYDET_REC_TOPK, keys, stream)
                   : launch_postprocess<4>(p, a.bbox, a.cidx, a.score, B, N, conf, nms_thres, MYDET_REC_TOPK, keys, stream);
    if (rotated_nms) return launch_postprocess<5, true>(p, a.bbox, a.cidx, a.score, B, N, conf, nms_thres, MYDET_REC_TOPK, keys, stream);
    return metric == MYDET_MERGE_IOS
               ? launch_postprocess<5, false, true>(p, a.bbox, a.cidx, a.score, B, N, conf, nms_thres, MYDET_REC_TOPK, keys, stream)
               : launch_postprocess<5>(p, a.bbox, a.cidx, a.score, B, N, conf, nms_thres, MYDET_REC_TOPK, keys, stream);
}

// agnostic: the merge's NMS has one group of all candidates (mydet_merge_tile_records_nms_f32); 0 is the shipped call
static int merge_tile_records(const int32_t *tile_records, int64_t tile_stride_words, int64_t frame_stride_words,
                              int B, int T, int box_width, const int32_t *origins, double nms_thres, int metric,
                              int rotated_nms, int agnostic, int32_t *records, void *scratch, int64_t scratch_bytes, void *stream) {
    const int bad = merge_check_args(tile_records, tile_stride_words, frame_stride_words, B, T, MYDET_TILES_MAX, box_width, origins, metric,
                                     rotated_nms, agnostic, records, scratch);
    if (bad) return bad;
    if (scratch_bytes < mydet_merge_tile_records_scratch_bytes(B, T, box_width)) return MYDET_E_BADARG;
    if (metric == MYDET_MERGE_IOS && rotated_nms) return MYDET_E_UNSUPP;
    if (agnostic && rotated_nms) return MYDET_E_UNSUPP;
    const int64_t N = (int64_t)T * KMAX;
    MergeArgs a = {};
    a.rec = tile_records; a.tile_st = tile_stride_words; a.frame_st = frame_stride_words; a.origins = origins; a.T = T;
    void *keys = merge_layout(a, scratch, (int64_t)B * N, box_width);
    const dim3 grid((unsigned)(N / 256), (unsigned)B);
    if (box_width == 4) hipLaunchKernelGGL((merge_gather_kernel<4>), grid, dim3(256), 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL((merge_gather_kernel<5>), grid, dim3(256), 0, (hipStream_t)stream, a);
    const int st = mydet_launch_status();
    if (st) return st;
    return merge_nms(a, B, N, box_width, nms_thres, metric, rotated_nms, agnostic, records, keys, stream);
}

extern "C" int mydet_merge_tile_records_f32(const int32_t *tile_records, int64_t tile_stride_words, int64_t frame_stride_words,
                                            int B, int T, int box_width, const int32_t *origins, double nms_thres, int metric,
                                            int rotated_nms, int32_t *records, void *scratch, int64_t scratch_bytes, void *stream) {
    return merge_tile_records(tile_records, tile_stride_words, frame_stride_words, B, T, box_width, origins, nms_thres, metric,
                              rotated_nms, 0, records, scratch, scratch_bytes, stream);
}

extern "C" int mydet_merge_tile_records_nms_f32(const int32_t *tile_records, int64_t tile_stride_words, int64_t frame_stride_words,
                                                int B, int T, int box_width, const int32_t *origins, double nms_thres, int metric,
                                                int rotated_nms, int agnostic, int32_t *records, void *scratch,
                                                int64_t scratch_bytes, void *stream) {
    return merge_tile_records(tile_records, tile_stride_words, frame_stride_words, B, T, box_width, origins, nms_thres, metric,
                              rotated_nms, agnostic, records, scratch, scratch_bytes, stream);
}

// ---- fusion of view records (test-time augmentation; include/mydet.h) ----
// The detector ran on V mirrored (and possibly rescaled) views of each frame; the records of the views, already in the pixel
// coordinates of the mirrored frame, become one record per frame.  The gather above (VIEW instances) brings every box back from
// its view and writes the B x V*512 candidate arrays.  MYDET_FUSE_NMS then runs postprocess_kernel on them exactly as the merge
// of tile records does.  MYDET_FUSE_WBF runs wbf_kernel: Weighted Boxes Fusion (Solovyev et al. 2021) with the rules of the
// header -- every candidate, in order P, joins the cluster whose running fused box it overlaps most, or founds one.
namespace {

constexpr int WBF_NMAX = MYDET_VIEWS_MAX * KMAX;

struct WbfArgs {
    PPArgs o;                         // the record outputs (write_row / finish_rows)
    const float *bbox;                // the gathered candidates: [B][N][4], [B][N], [B][N]
    const int64_t *cidx;
    const float *score;
    int N, V, agn;
    double thres;
    float min_score;
};

// LDS of wbf_kernel, dynamic (66 KiB + the scalars: above the 64 KiB a kernel gets without the opt-in)
struct WbfLds {
    unsigned long long key[WBF_NMAX];  // the candidates in order P; afterwards the first KMAX hold the output order keys
    double sum[5][KMAX];               // Wt, X1, Y1, X2, Y2 of cluster j
    float f[4][KMAX];                  // its fused row (cx, cy, w, h)
    int n[KMAX], cls[KMAX], first[KMAX];
    int nvalid, bad, ncl, total;
};

__device__ __forceinline__ float wbf_lane(float v, int lane) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane)); }
__device__ __forceinline__ unsigned long long wbf_lane64u(unsigned long long u, int lane) {
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)u, lane), hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(u >> 32), lane);
    return ((unsigned long long)hi << 32) | lo;
}
__device__ __forceinline__ double wbf_lane64(double v, int lane) {
    return __longlong_as_double((long long)wbf_lane64u((unsigned long long)__double_as_longlong(v), lane));
}

// One workgroup per frame.  All 16 waves build and sort the keys and write the output; the clustering itself is one dependent
// chain over the candidates (a candidate's match depends on every fused box before it, and the 512-cluster cap ties the classes
// together), so wave 0 walks it alone: a lane owns clusters lane, lane + 64, ..., the match of a candidate is one wave maximum
// over (IoU, lowest j), and lanes 0-4 update the five sums of the matched cluster (one division for the four means).  64 candidates at a time are fetched into registers and handed
// round with v_readlane, so the chain waits for memory once per 64 steps.
__global__ __launch_bounds__(NT) void wbf_kernel(const WbfArgs p) {
    extern __shared__ __align__(16) unsigned char wbf_raw[];
    WbfLds &s = *reinterpret_cast<WbfLds *>(wbf_raw);
    const int tid = threadIdx.x, b = blockIdx.x, N = p.N;
    const float *bb = p.bbox + (int64_t)b * N * 4;
    const int64_t *ci = p.cidx + (int64_t)b * N;
    const float *sc = p.score + (int64_t)b * N;
    int npow = KMAX;                                        // keys sorted: the power of two that holds N
    while (npow < N) npow <<= 1;

    if (tid == 0) { s.nvalid = 0; s.bad = 0; s.ncl = 0; s.total = 0; }
    __syncthreads();
    // 1. keys of the candidates with a score > 0 (a NaN -- every slot past a view's count -- fails the test): ~score, then index
    for (int i = tid; i < npow; i += NT) {
        unsigned long long k = ~0ull;
        if (i < N) {
            const float v = sc[i];
            if (v > 0.0f) {
                if ((unsigned long long)ci[i] > 0xFFFull) s.bad = 1;       // the bad-class sentinel of a view, or a class the keys cannot hold
                k = ((unsigned long long)(~sortable(v)) << 12) | (unsigned long long)i;
                atomicAdd(&s.nvalid, 1);
            }
        }
        s.key[i] = k;
    }
    __syncthreads();
    for (int k = 2; k <= npow; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < npow; i += NT) {
                const int ixj = i ^ j;
                if (ixj > i) {
                    const unsigned long long x = s.key[i], c = s.key[ixj];
                    const bool up = (i & k) == 0;
                    if ((x > c) == up) { s.key[i] = c; s.key[ixj] = x; }
                }
            }
            __syncthreads();
        }
    }
    const int nvalid = s.nvalid;
    const bool bad = s.bad != 0;

    // 2. the chain
    if (tid < 64 && !bad) {
        const int lane = tid;
        int ncl = 0;
        for (int base = 0; base < nvalid; base += 64) {
            float x1 = 0.f, y1 = 0.f, x2 = 0.f, y2 = 0.f, ar = 0.f, cs = 0.f;
            int cq = 0, cidx = 0;
            if (base + lane < nvalid) {
                cidx = (int)(s.key[base + lane] & 4095ull);
                const f32x4 v = *reinterpret_cast<const f32x4 *>(bb + (int64_t)cidx * 4);
                const float hw = v[2] / 2.0f, hh = v[3] / 2.0f;
                x1 = v[0] - hw; y1 = v[1] - hh; x2 = v[0] + hw; y2 = v[1] + hh;
                ar = (x2 - x1) * (y2 - y1);
                cs = sc[cidx];
                cq = (int)ci[cidx];
            }
            const int nb = min(64, nvalid - base);
            for (int i = 0; i < nb; ++i) {
                const float bx1 = wbf_lane(x1, i), by1 = wbf_lane(y1, i), bx2 = wbf_lane(x2, i), by2 = wbf_lane(y2, i);
                const float ba = wbf_lane(ar, i), bs = wbf_lane(cs, i);
                const int q_cls = __builtin_amdgcn_readlane(cq, i), idx = __builtin_amdgcn_readlane(cidx, i);
                unsigned long long best = 0ull;            // (sortable IoU, ~j) of the best eligible cluster above the threshold
                for (int j = lane; j < ncl; j += 64) {
                    if (!p.agn && s.cls[j] != q_cls) continue;
                    const float fw = s.f[2][j] / 2.0f, fh = s.f[3][j] / 2.0f;
                    const float jx1 = s.f[0][j] - fw, jy1 = s.f[1][j] - fh, jx2 = s.f[0][j] + fw, jy2 = s.f[1][j] + fh;
                    const float o = pair_iou(jx1, jy1, jx2, jy2, (jx2 - jx1) * (jy2 - jy1), bx1, by1, bx2, by2, ba);
                    if ((double)o > p.thres) {             // false for a NaN
                        const unsigned long long k = ((unsigned long long)sortable(o) << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)j);
                        best = k > best ? k : best;
                    }
                }
                // the wave maximum.  Most steps have no lane above the threshold (a founder) or exactly one (a box of an object
                // the views agree on): those read the answer from the ballot, and only a contested step pays the six shuffle rounds
                const unsigned long long hit = __ballot(best != 0ull);
                if (hit != 0ull && (hit & (hit - 1ull)) == 0ull) {
                    best = wbf_lane64u(best, __ffsll((long long)hit) - 1);
                } else if (hit != 0ull) {
#pragma unroll
                    for (int off = 32; off >= 1; off >>= 1) {
                        const unsigned long long o = __shfl_xor(best, off);
                        best = o > best ? o : best;
                    }
                }
                int j = -1;                                 // uniform from here on
                if (best != 0ull) j = (int)(0xFFFFFFFFu - (unsigned)(best & 0xFFFFFFFFull));
                else if (ncl < KMAX) j = ncl;
                if (j >= 0) {
                    // lane l < 5 owns sum l of the cluster (Wt, X1, Y1, X2, Y2), so the five updates are one instruction stream and
                    // the four quotients one division; lane 0 then writes the fused row
                    const bool found = best == 0ull;
                    const float mine = lane == 1 ? bx1 : lane == 2 ? by1 : lane == 3 ? bx2 : lane == 4 ? by2 : 1.0f;
                    double acc = 0.0;
                    if (lane < 5) {
                        acc = (found ? 0.0 : s.sum[lane][j]) + (double)bs * (double)mine;      // lane 0: s * 1 = s exactly
                        s.sum[lane][j] = acc;
                    }
                    const double q = acc / wbf_lane64(acc, 0);
                    const double mx1 = wbf_lane64(q, 1), my1 = wbf_lane64(q, 2), mx2 = wbf_lane64(q, 3), my2 = wbf_lane64(q, 4);
                    if (lane == 0) {
                        s.f[0][j] = (float)((mx1 + mx2) * 0.5); s.f[1][j] = (float)((my1 + my2) * 0.5);
                        s.f[2][j] = (float)(mx2 - mx1); s.f[3][j] = (float)(my2 - my1);
                        if (found) { s.n[j] = 1; s.cls[j] = q_cls; s.first[j] = idx; }
                        else s.n[j] = s.n[j] + 1;
                    }
                }
                if (best == 0ull && ncl < KMAX) ++ncl;
                __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");     // lane 0's cluster is what every lane reads next
            }
        }
        if (lane == 0) s.ncl = ncl;
    }
    __syncthreads();

    // 3. scores, the min_score cut, the output order (class ascending, score descending, creation order) and the rows
    const int ncl = s.ncl;
    float fs = 0.f;
    unsigned long long ok = ~0ull;
    if (tid < ncl) {
        const int n = s.n[tid];
        fs = (float)((s.sum[0][tid] / (double)n) * ((double)min(n, p.V) / (double)p.V));
        if (!(fs < p.min_score))
            ok = ((unsigned long long)s.cls[tid] << 41) | ((unsigned long long)(~sortable(fs)) << 9) | (unsigned long long)tid;
    }
    if (tid < KMAX) s.key[tid] = ok;                        // every candidate key has been read: the chain is over
    __syncthreads();
    bitonic_sort_kmax(s.key, tid);
    if (tid < KMAX && s.key[tid] != ~0ull && (tid == KMAX - 1 || s.key[tid + 1] == ~0ull)) s.total = tid + 1;
    __syncthreads();
    const int total = bad ? 0 : s.total;
    if (tid < total) {
        const int j = (int)(s.key[tid] & (KMAX - 1));
        const int n = s.n[j];
        const float f = (float)((s.sum[0][j] / (double)n) * ((double)min(n, p.V) / (double)p.V));
        write_row<4>(p.o, b, tid, f32x4{s.f[0][j], s.f[1][j], s.f[2][j], s.f[3][j]}, 0.f, (int64_t)s.cls[j], f, (unsigned)s.first[j]);
    }
    finish_rows<4>(p.o, b, total, bad, tid);
}

}  // namespace

extern "C" int64_t mydet_fuse_view_records_scratch_bytes(int B, int V, int box_width, int kind) {
    if (B <= 0 || V < 1 || V > MYDET_VIEWS_MAX || (box_width != 4 && box_width != 5)) return 0;
    if (kind == MYDET_FUSE_NMS) return (int64_t)B * V * KMAX * (4 * box_width + 8 + 4 + 8);
    if (kind == MYDET_FUSE_WBF && box_width == 4) return (int64_t)B * V * KMAX * (16 + 8 + 4);    // no key strip
    return 0;
}

extern "C" int mydet_fuse_view_records_f32(const int32_t *view_records, int64_t view_stride_words, int64_t frame_stride_words,
                                           int B, int V, int box_width, const int32_t *flips, int frame_h, int frame_w,
                                           double thres, const mydet_fuse_mode *mode, int32_t *records,
                                           void *scratch, int64_t scratch_bytes, void *stream) {
    if (!mode || (mode->kind != MYDET_FUSE_NMS && mode->kind != MYDET_FUSE_WBF)) return MYDET_E_BADARG;
    const int bad = merge_check_args(view_records, view_stride_words, frame_stride_words, B, V, MYDET_VIEWS_MAX, box_width, flips,
                                     mode->metric, mode->rotated_nms, mode->agnostic, records, scratch);
    if (bad) return bad;
    if (frame_h <= 0 || frame_w <= 0 || !(mode->min_score >= 0.0f)) return MYDET_E_BADARG;
    unsigned packed = 0u;
    for (int v = 0; v < V; ++v) {
        if (flips[v] < 0 || flips[v] > (MYDET_VIEW_HFLIP | MYDET_VIEW_VFLIP)) return MYDET_E_BADARG;
        packed |= (unsigned)flips[v] << (2 * v);
    }
    const bool wbf = mode->kind == MYDET_FUSE_WBF;
    if (wbf && (box_width != 4 || mode->metric != MYDET_MERGE_IOU || mode->rotated_nms)) return MYDET_E_UNSUPP;
    if (!wbf && mode->rotated_nms && (mode->metric == MYDET_MERGE_IOS || mode->agnostic)) return MYDET_E_UNSUPP;
    if (scratch_bytes < mydet_fuse_view_records_scratch_bytes(B, V, box_width, mode->kind)) return MYDET_E_BADARG;
    const int64_t N = (int64_t)V * KMAX;
    MergeArgs a = {};
    a.rec = view_records; a.tile_st = view_stride_words; a.frame_st = frame_stride_words; a.origins = nullptr; a.T = V;
    a.flips = packed; a.frame_w = (float)frame_w; a.frame_h = (float)frame_h; a.zero_origin = wbf ? 0 : 1;
    void *keys = merge_layout(a, scratch, (int64_t)B * N, box_width);
    static unsigned long long opted = 0ull;
    if (wbf) {
        const int st = mydet_lds_opt_in(opted, wbf_kernel, (int)sizeof(WbfLds));
        if (st) return st;
    }
    const dim3 grid((unsigned)(N / 256), (unsigned)B);
    if (box_width == 4) hipLaunchKernelGGL((merge_gather_kernel<4, true>), grid, dim3(256), 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL((merge_gather_kernel<5, true>), grid, dim3(256), 0, (hipStream_t)stream, a);
    const int st = mydet_launch_status();
    if (st) return st;
    if (!wbf)
        return merge_nms(a, B, N, box_width, thres, mode->metric, mode->rotated_nms, mode->agnostic, records, keys, stream);
    WbfArgs w = {};
    record_outputs(w.o, records, false);
    w.o.topk = MYDET_REC_TOPK;
    w.bbox = a.bbox; w.cidx = a.cidx; w.score = a.score; w.N = (int)N; w.V = V; w.agn = mode->agnostic;
    w.thres = thres; w.min_score = mode->min_score;
    hipLaunchKernelGGL(wbf_kernel, dim3(B), dim3(NT), sizeof(WbfLds), (hipStream_t)stream, w);
    return mydet_launch_status();
}
