// HOTA (Luiten et al., IJCV 2021) on the device, over the packed arrays of include/mydet.h (mydet_eval_set with frames as images and
// mydet_mot_set beside it; the rules are there, "HOTA", and in DESIGN.md section 4).  The pair values are the output of
// mydet_eval_ious_f64, unchanged.
//   mydet_hota_align_f64   one thread per row for the presence counts; one workgroup per listed group for the alignment scores:
//                          row and column sums in LDS (fixed order), then one int64 atomic add per pair into the potentials
//   mydet_hota_match       one wavefront per listed group: the pair scores q once per pair, then hung_solve (hung.h) on 2^20 - q
//   mydet_hota_score_f64   one thread per matched row: integer atomic adds into the match-count matrices; then one workgroup per
//                          (unit, alpha): TP / FN / FP, the IoU sum and the three association sums
// A frame's assignment carries no state and does not depend on alpha, so every frame of every sequence is one independent
// wavefront.  Every decision is an integer or a float64 comparison and every accumulation that feeds one is fixed point, so no
// order of evaluation can change it; the two float64 sums (loc_sum, ass_sum) are added per thread in index order and then by a
// fixed tree, so they repeat from run to run.  Built with -ffp-contract=off like mot.hip.
#include "common.h"
#include "eval_set.h"
#include "hung.h"

namespace {

constexpr int HOTA_BLOCK = 256;
constexpr int HOTA_MAX_FRAMES = 1 << 22;         // (gt_count + dt_count) * 2^30 stays below 2^53
constexpr double HOTA_P_ONE = 1073741824.0;      // 2^30: one frame of perfect alignment in a potential
constexpr int32_t HOTA_Q_ONE = 1048576;          // 2^20: the pair score of a perfect pair
static_assert(MYDET_EVAL_MAX_GT == MYDET_EVAL_MAX_DT, "one HungLds serves both orientations");

struct HotaAlphas {                              // host array, copied into the launch
    double a[MYDET_EVAL_MAX_THRS];
    int T;
};

struct HotaUnit {
    int n_gid, n_hid, gid0, hid0;
    int64_t ov;
    bool ok;                                     // its tables hold what was promised and lie inside the arrays
};

__device__ __forceinline__ HotaUnit hota_unit(const mydet_mot_set &m, int u) {
    HotaUnit t;
    t.gid0 = m.gt_id_start[u];
    t.n_gid = m.gt_id_start[u + 1] - t.gid0;
    t.hid0 = m.dt_id_start[u];
    t.n_hid = m.dt_id_start[u + 1] - t.hid0;
    t.ov = m.ov_start[u];
    t.ok = t.n_gid >= 0 && t.n_gid <= MYDET_MOT_MAX_IDS && t.n_hid >= 0 && t.n_hid <= MYDET_MOT_MAX_IDS && t.gid0 >= 0 && t.hid0 >= 0 &&
           (int64_t)t.gid0 + t.n_gid <= m.n_gt_ids && (int64_t)t.hid0 + t.n_hid <= m.n_dt_ids && t.ov >= 0 &&
           t.ov + (int64_t)t.n_gid * t.n_hid <= m.n_ov;
    return t;
}

// The unit of group g: its category and the last sequence with seq_start <= its frame.
__device__ __forceinline__ int hota_unit_of(const mydet_eval_set &s, const mydet_mot_set &m, int g) {
    const int k = g / s.I, f = g - k * s.I;
    int a = 0, b = m.S;
    while (b - a > 1) {
        const int mid = (a + b) >> 1;
        if (m.seq_start[mid] <= f) a = mid; else b = mid;
    }
    return k * m.S + a;
}

struct HotaGroup {
    int d0, nd, g0, ng, c;                       // c: the listed position when both sides are non-empty
    bool ok;                                     // takes part: inside the caps and the arrays, and listed when it has pairs
};

__device__ __forceinline__ HotaGroup hota_group(const mydet_eval_set &s, int g) {
    HotaGroup r;
    r.d0 = s.dt_start[g];
    r.nd = s.dt_start[g + 1] - r.d0;
    r.g0 = s.gt_start[g];
    r.ng = s.gt_start[g + 1] - r.g0;
    r.c = -1;
    r.ok = r.nd >= 0 && r.ng >= 0 && r.nd <= MYDET_EVAL_MAX_DT && r.ng <= MYDET_EVAL_MAX_GT && r.d0 >= 0 && r.g0 >= 0 &&
           (int64_t)r.d0 + r.nd <= s.D && (int64_t)r.g0 + r.ng <= s.G;
    if (r.ok && r.nd > 0 && r.ng > 0) {
        int lo = 0, hi = s.n_groups;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (s.groups[mid] < g) lo = mid + 1; else hi = mid;
        }
        r.c = lo < s.n_groups && s.groups[lo] == g ? lo : -1;
        r.ok = r.c >= 0 && s.pair_start[r.c] >= 0 && s.pair_start[r.c] + (int64_t)r.nd * r.ng <= s.n_pairs;
    }
    return r;
}

// The group of a row of one side: the last g in [lo, hi) with start[g] <= row (empty groups before it share its start).
__device__ __forceinline__ int hota_group_of_row(const int32_t *start, int lo, int hi, int64_t row) {
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (start[mid] <= row) lo = mid; else hi = mid;
    }
    return lo;
}

// A NaN pair value counts as 0.
__device__ __forceinline__ double hota_iou(double v) { return v != v ? 0.0 : v; }

// gt_count and dt_count: one thread per row of either side.
__global__ __launch_bounds__(HOTA_BLOCK) void hota_count_kernel(const mydet_eval_set s, const mydet_mot_set m, int32_t *gt_count,
                                                                int32_t *dt_count) {
    const int n_g = s.I * s.K;
    for (int64_t e = (int64_t)blockIdx.x * HOTA_BLOCK + threadIdx.x; e < s.G + s.D; e += (int64_t)gridDim.x * HOTA_BLOCK) {
        const bool is_gt = e < s.G;
        const int64_t row = is_gt ? e : e - s.G;
        const int g = hota_group_of_row(is_gt ? s.gt_start : s.dt_start, 0, n_g, row);
        const HotaGroup gr = hota_group(s, g);
        if (!gr.ok || row < (is_gt ? gr.g0 : gr.d0) || row >= (is_gt ? gr.g0 + gr.ng : gr.d0 + gr.nd)) continue;
        const HotaUnit un = hota_unit(m, hota_unit_of(s, m, g));
        if (!un.ok) continue;
        const int id = is_gt ? m.gt_id[row] : m.dt_id[row];
        if ((unsigned)id >= (unsigned)(is_gt ? un.n_gid : un.n_hid)) continue;
        atomicAdd(is_gt ? gt_count + un.gid0 + id : dt_count + un.hid0 + id, 1);
    }
}

// Rule 1 for one listed group with both sides non-empty.
__global__ __launch_bounds__(HOTA_BLOCK) void hota_align_kernel(const mydet_eval_set s, const mydet_mot_set m, const double *ious,
                                                                int64_t *pot) {
    __shared__ double rowsum[MYDET_EVAL_MAX_GT], colsum[MYDET_EVAL_MAX_DT];
    const int tid = threadIdx.x, c = blockIdx.x;
    const int g = s.groups[c];
    if (g < 0 || g >= s.I * s.K) return;
    const HotaGroup gr = hota_group(s, g);
    if (!gr.ok || gr.c != c) return;                                   // gr.c == c: both sides non-empty
    const HotaUnit un = hota_unit(m, hota_unit_of(s, m, g));
    if (!un.ok) return;
    const int nd = gr.nd, ng = gr.ng;
    const double *iou = ious + s.pair_start[c];
    for (int r = tid; r < ng; r += HOTA_BLOCK) {
        double sum = 0.0;
        for (int j = 0; j < nd; ++j) sum += hota_iou(iou[(int64_t)j * ng + r]);
        rowsum[r] = sum;
    }
    for (int j = tid; j < nd; j += HOTA_BLOCK) {
        double sum = 0.0;
        for (int r = 0; r < ng; ++r) sum += hota_iou(iou[(int64_t)j * ng + r]);
        colsum[j] = sum;
    }
    __syncthreads();
    for (int p = tid; p < nd * ng; p += HOTA_BLOCK) {
        const int j = p / ng, r = p - j * ng;
        const double v = iou[p];
        if (!(v > 0.0)) continue;                                      // NaN too
        const double den = rowsum[r] + colsum[j] - v;
        const double sc = v / den;
        if (!(sc >= 0.0 && sc <= 1.0)) continue;                       // pair values outside [0, 1]: nothing is added
        const int64_t add = (int64_t)floor(sc * HOTA_P_ONE);
        const int o = m.gt_id[gr.g0 + r], h = m.dt_id[gr.d0 + j];
        if (add == 0 || (unsigned)o >= (unsigned)un.n_gid || (unsigned)h >= (unsigned)un.n_hid) continue;
        atomicAdd(reinterpret_cast<unsigned long long *>(pot + un.ov + (int64_t)o * un.n_hid + h), (unsigned long long)add);
    }
}

struct HotaCost {
    const int32_t *q;                            // the group's block: [column (hypothesis)][row (ground truth)]
    int ng;
    bool transposed;                             // the routine's rows are the columns
    __device__ __forceinline__ int64_t operator()(int i, int j) const {
        const int r = transposed ? j : i, c = transposed ? i : j;
        return (int64_t)(HOTA_Q_ONE - q[(int64_t)c * ng + r]);
    }
};

// Rules 2 and 3 for one listed group with both sides non-empty: one wavefront.
__global__ __launch_bounds__(MOT_WAVE) void hota_match_kernel(const mydet_eval_set s, const mydet_mot_set m, const double *ious,
                                                              const int64_t *pot, const int32_t *gt_count, const int32_t *dt_count,
                                                              int32_t *score_q, int32_t *match) {
    extern __shared__ __align__(16) unsigned char hota_raw[];
    HungLds<MYDET_EVAL_MAX_GT> &L = *reinterpret_cast<HungLds<MYDET_EVAL_MAX_GT> *>(hota_raw);
    const int lane = threadIdx.x, c = blockIdx.x;
    const int g = s.groups[c];
    if (g < 0 || g >= s.I * s.K) return;
    const HotaGroup gr = hota_group(s, g);
    if (!gr.ok || gr.c != c) return;
    const HotaUnit un = hota_unit(m, hota_unit_of(s, m, g));
    if (!un.ok) return;
    const int nd = gr.nd, ng = gr.ng;
    const double *iou = ious + s.pair_start[c];
    int32_t *q = score_q + s.pair_start[c];
    for (int p = lane; p < nd * ng; p += MOT_WAVE) {
        const int j = p / ng, r = p - j * ng;
        const int o = m.gt_id[gr.g0 + r], h = m.dt_id[gr.d0 + j];
        int32_t qv = 0;
        if ((unsigned)o < (unsigned)un.n_gid && (unsigned)h < (unsigned)un.n_hid) {
            const int64_t P = pot[un.ov + (int64_t)o * un.n_hid + h];
            const int64_t den = ((int64_t)gt_count[un.gid0 + o] + (int64_t)dt_count[un.hid0 + h]) * (int64_t)1073741824 - P;
            if (P > 0 && den > 0) {
                const double A = (double)P / (double)den;
                const double x = floor(A * hota_iou(iou[p]) * 1048576.0);
                qv = x >= 0.0 && x <= 1048576.0 ? (int32_t)x : 0;      // pair values outside [0, 1]: no score
            }
        }
        q[p] = qv;
    }
    __syncthreads();                                                   // the scores are read back by other lanes
    HotaCost cost = {q, ng, ng > nd};
    const int hn = cost.transposed ? nd : ng, hm = cost.transposed ? ng : nd;
    hung_solve(L, hn, hm, cost, lane);
    for (int j = lane; j < hm; j += MOT_WAVE) {
        const int i = L.p[j];
        if (i < 0) continue;
        const int r = cost.transposed ? j : i, cc = cost.transposed ? i : j;
        match[gr.g0 + r] = gr.d0 + cc;
    }
}

// Rule 4, the match counts: one thread per ground-truth row.
__global__ __launch_bounds__(HOTA_BLOCK) void hota_tp_kernel(const mydet_eval_set s, const mydet_mot_set m, const HotaAlphas q,
                                                             const double *ious, const int32_t *match, int32_t *matches) {
    const int n_g = s.I * s.K;
    for (int64_t row = (int64_t)blockIdx.x * HOTA_BLOCK + threadIdx.x; row < s.G; row += (int64_t)gridDim.x * HOTA_BLOCK) {
        const int hm = match[row];
        if (hm < 0) continue;
        const int g = hota_group_of_row(s.gt_start, 0, n_g, row);
        const HotaGroup gr = hota_group(s, g);
        if (!gr.ok || gr.c < 0 || row < gr.g0 || row >= gr.g0 + gr.ng || hm < gr.d0 || hm >= gr.d0 + gr.nd) continue;
        const HotaUnit un = hota_unit(m, hota_unit_of(s, m, g));
        if (!un.ok) continue;
        const int o = m.gt_id[row], h = m.dt_id[hm];
        if ((unsigned)o >= (unsigned)un.n_gid || (unsigned)h >= (unsigned)un.n_hid) continue;
        const double v = ious[s.pair_start[gr.c] + (int64_t)(hm - gr.d0) * gr.ng + (row - gr.g0)];
        const int64_t at = un.ov + (int64_t)o * un.n_hid + h;
        for (int t = 0; t < q.T; ++t)
            if (v >= q.a[t]) atomicAdd(matches + (int64_t)t * m.n_ov + at, 1);
    }
}

// Thread sums, thread 0 ... HOTA_BLOCK - 1 -> their sum in every thread, by a fixed tree.
template <typename V>
__device__ __forceinline__ V hota_block_sum(V x, V *lds) {
    const int tid = threadIdx.x;
    __syncthreads();
    lds[tid] = x;
    __syncthreads();
    for (int half = HOTA_BLOCK / 2; half > 0; half >>= 1) {
        if (tid < half) lds[tid] = lds[tid] + lds[tid + half];
        __syncthreads();
    }
    return lds[0];
}

// Rule 4 for one (unit, alpha).
__global__ __launch_bounds__(HOTA_BLOCK) void hota_sum_kernel(const mydet_eval_set s, const mydet_mot_set m, const HotaAlphas q,
                                                              const double *ious, const int32_t *match, const int32_t *gt_count,
                                                              const int32_t *dt_count, const int32_t *matches, int64_t *counts,
                                                              double *loc_sum, double *ass_sum) {
    __shared__ double lds_f[HOTA_BLOCK];
    __shared__ int64_t lds_i[HOTA_BLOCK];
    const int tid = threadIdx.x;
    const int u = blockIdx.x / q.T, t = blockIdx.x - u * q.T;
    const int k = u / m.S, sq = u - k * m.S;
    const double alpha = q.a[t];
    const HotaUnit un = hota_unit(m, u);
    const int f0 = max(m.seq_start[sq], 0), f1 = min(m.seq_start[sq + 1], s.I);
    int64_t rows = 0, cols = 0, tp = 0;
    double loc = 0.0, a0 = 0.0, a1 = 0.0, a2 = 0.0;
    if (un.ok && f1 > f0) {
        const int ga = k * s.I + f0, gb = k * s.I + f1;
        for (int g = ga + tid; g < gb; g += HOTA_BLOCK) {              // the rows and columns of the groups that take part
            const HotaGroup gr = hota_group(s, g);
            if (!gr.ok) continue;
            rows += gr.ng;
            cols += gr.nd;
        }
        const int64_t r0 = s.gt_start[ga], r1 = s.gt_start[gb];
        for (int64_t row = max(r0, (int64_t)0) + tid; row < min(r1, s.G); row += HOTA_BLOCK) {
            const int hm = match[row];
            if (hm < 0) continue;
            const int g = hota_group_of_row(s.gt_start, ga, gb, row);
            const HotaGroup gr = hota_group(s, g);
            if (!gr.ok || gr.c < 0 || row < gr.g0 || row >= gr.g0 + gr.ng || hm < gr.d0 || hm >= gr.d0 + gr.nd) continue;
            const double v = ious[s.pair_start[gr.c] + (int64_t)(hm - gr.d0) * gr.ng + (row - gr.g0)];
            if (v >= alpha) {
                tp += 1;
                loc += v;
            }
        }
        const int32_t *M = matches + (int64_t)t * m.n_ov + un.ov;
        const int n_ent = un.n_gid * un.n_hid;
        for (int i = tid; i < n_ent; i += HOTA_BLOCK) {
            const int mv = M[i];
            if (mv <= 0) continue;
            const int o = i / un.n_hid, h = i - o * un.n_hid;
            const int gc = gt_count[un.gid0 + o], dc = dt_count[un.hid0 + h];
            const double md = (double)mv;
            a0 += md * (md / (double)max(1, gc + dc - mv));
            a1 += md * (md / (double)max(1, gc));
            a2 += md * (md / (double)max(1, dc));
        }
    }
    rows = hota_block_sum(rows, lds_i);
    cols = hota_block_sum(cols, lds_i);
    tp = hota_block_sum(tp, lds_i);
    loc = hota_block_sum(loc, lds_f);
    a0 = hota_block_sum(a0, lds_f);
    a1 = hota_block_sum(a1, lds_f);
    a2 = hota_block_sum(a2, lds_f);
    if (tid == 0) {
        const int64_t at = (int64_t)u * q.T + t;
        counts[at * 3 + 0] = tp;
        counts[at * 3 + 1] = rows - tp;
        counts[at * 3 + 2] = cols - tp;
        loc_sum[at] = loc;
        ass_sum[at * 3 + 0] = a0;
        ass_sum[at * 3 + 1] = a1;
        ass_sum[at * 3 + 2] = a2;
    }
}

int hota_check(const mydet_eval_set *s, const mydet_mot_set *m) {
    const int code = mot_check(s, m);
    if (code) return code;
    return s->I > HOTA_MAX_FRAMES ? MYDET_E_UNSUPP : 0;
}

int hota_alphas(HotaAlphas &q, const double *alphas, int T) {
    if (!alphas || T < 1) return MYDET_E_BADARG;
    if (T > MYDET_EVAL_MAX_THRS) return MYDET_E_UNSUPP;
    for (int t = 0; t < T; ++t) {
        if (!(alphas[t] > 0.0 && alphas[t] <= 1.0)) return MYDET_E_BADARG;   // NaN too
        q.a[t] = alphas[t];
    }
    q.T = T;
    return 0;
}

unsigned hota_grid(int64_t threads) {
    int64_t blocks = (threads + HOTA_BLOCK - 1) / HOTA_BLOCK;
    if (blocks > 256 * 16) blocks = 256 * 16;
    return (unsigned)blocks;
}

}  // namespace

extern "C" int mydet_hota_align_f64(const mydet_eval_set *set, const mydet_mot_set *mot, const double *ious, int64_t *pot,
                                    int32_t *gt_count, int32_t *dt_count, void *stream) {
    const int code = hota_check(set, mot);
    if (code) return code;
    if ((set->n_pairs > 0 && !ious) || (mot->n_ov > 0 && !pot) || (mot->n_gt_ids > 0 && !gt_count) || (mot->n_dt_ids > 0 && !dt_count))
        return MYDET_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    if (mot->n_ov > 0 && hipMemsetAsync(pot, 0, (size_t)mot->n_ov * sizeof(int64_t), st) != hipSuccess) return mydet_launch_status();
    if (mot->n_gt_ids > 0 && hipMemsetAsync(gt_count, 0, (size_t)mot->n_gt_ids * sizeof(int32_t), st) != hipSuccess) return mydet_launch_status();
    if (mot->n_dt_ids > 0 && hipMemsetAsync(dt_count, 0, (size_t)mot->n_dt_ids * sizeof(int32_t), st) != hipSuccess) return mydet_launch_status();
    if (mot->n_gt_ids > 0 || mot->n_dt_ids > 0) {
        hipLaunchKernelGGL(hota_count_kernel, dim3(hota_grid(set->G + set->D)), dim3(HOTA_BLOCK), 0, st, *set, *mot, gt_count, dt_count);
        const int launched = mydet_launch_status();
        if (launched) return launched;
    }
    if (set->n_pairs == 0 || mot->n_ov == 0) return 0;
    hipLaunchKernelGGL(hota_align_kernel, dim3((unsigned)set->n_groups), dim3(HOTA_BLOCK), 0, st, *set, *mot, ious, pot);
    return mydet_launch_status();
}

extern "C" int mydet_hota_match(const mydet_eval_set *set, const mydet_mot_set *mot, const double *ious, const int64_t *pot,
                                const int32_t *gt_count, const int32_t *dt_count, int32_t *score_q, int32_t *hota_match, void *stream) {
    const int code = hota_check(set, mot);
    if (code) return code;
    if ((set->n_pairs > 0 && (!ious || !score_q)) || (set->G > 0 && !hota_match)) return MYDET_E_BADARG;
    if ((mot->n_ov > 0 && !pot) || (mot->n_gt_ids > 0 && !gt_count) || (mot->n_dt_ids > 0 && !dt_count)) return MYDET_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    if (set->G > 0 && hipMemsetAsync(hota_match, 0xff, (size_t)set->G * sizeof(int32_t), st) != hipSuccess) return mydet_launch_status();
    if (set->n_pairs == 0) return 0;
    if (hipMemsetAsync(score_q, 0, (size_t)set->n_pairs * sizeof(int32_t), st) != hipSuccess) return mydet_launch_status();
    hipLaunchKernelGGL(hota_match_kernel, dim3((unsigned)set->n_groups), dim3(MOT_WAVE), sizeof(HungLds<MYDET_EVAL_MAX_GT>), st, *set, *mot,
                       ious, pot, gt_count, dt_count, score_q, hota_match);
    return mydet_launch_status();
}

extern "C" int mydet_hota_score_f64(const mydet_eval_set *set, const mydet_mot_set *mot, const double *ious, const int32_t *hota_match,
                                    const int32_t *gt_count, const int32_t *dt_count, const double *alphas, int T, int64_t *counts,
                                    int32_t *matches, double *loc_sum, double *ass_sum, void *stream) {
    const int code = hota_check(set, mot);
    if (code) return code;
    HotaAlphas q = {};
    const int bad = hota_alphas(q, alphas, T);
    if (bad) return bad;
    if (!counts || !loc_sum || !ass_sum || (mot->n_ov > 0 && !matches) || (set->n_pairs > 0 && !ious) || (set->G > 0 && !hota_match))
        return MYDET_E_BADARG;
    if ((mot->n_gt_ids > 0 && !gt_count) || (mot->n_dt_ids > 0 && !dt_count)) return MYDET_E_BADARG;
    const int64_t blocks = (int64_t)mot->S * set->K * T;
    if (blocks > 0x7fffffff) return MYDET_E_UNSUPP;
    hipStream_t st = (hipStream_t)stream;
    if (mot->n_ov > 0) {
        if (hipMemsetAsync(matches, 0, (size_t)mot->n_ov * T * sizeof(int32_t), st) != hipSuccess) return mydet_launch_status();
        if (set->n_pairs > 0) {
            hipLaunchKernelGGL(hota_tp_kernel, dim3(hota_grid(set->G)), dim3(HOTA_BLOCK), 0, st, *set, *mot, q, ious, hota_match, matches);
            const int launched = mydet_launch_status();
            if (launched) return launched;
        }
    }
    hipLaunchKernelGGL(hota_sum_kernel, dim3((unsigned)blocks), dim3(HOTA_BLOCK), 0, st, *set, *mot, q, ious, hota_match, gt_count, dt_count,
                       matches, counts, loc_sum, ass_sum);
    return mydet_launch_status();
}
