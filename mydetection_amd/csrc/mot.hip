// Track scoring on the device: the CLEAR MOT counts and the identity (IDF1) counts over the packed arrays of include/mydet.h
// (mydet_eval_set with frames as images, and mydet_mot_set beside it; the rules are there and in DESIGN.md section 4).  The pair
// values are the output of mydet_eval_ious_f64, unchanged.
//   mydet_mot_clear_f64    one wavefront per (unit, threshold): walks the unit's frames in order (keep, assign, count)
//   mydet_mot_id_overlap   one thread per IoU pair: integer atomic adds into the identity-overlap matrices
//   mydet_mot_id_assign    one wavefront per (unit, threshold): the largest one-to-one sum of overlaps
// Both wavefront kernels share hung_solve (hung.h), the shortest-augmenting-path Hungarian method on integer costs: lanes own columns
// (column j is lane j % 64), a row step is one wave minimum over (minv, column), and the costs are formed from the IoU buffer or
// the overlap matrix on the fly.  Every decision is an integer or a float64 comparison, so no order of evaluation can change it;
// the only float64 sum (SIOU) is added in ascending row order by readlane.  Built with -ffp-contract=off like evalmatch.hip.
#include "common.h"
#include "eval_set.h"
#include "hung.h"

namespace {

struct MotThresholds {                           // host array, copied into the launch
    double iou[MYDET_EVAL_MAX_THRS];
    int T;
};

// The listed position of group g, or -1.
__device__ __forceinline__ int mot_listed(const mydet_eval_set &s, int g) {
    int lo = 0, hi = s.n_groups;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (s.groups[mid] < g) lo = mid + 1; else hi = mid;
    }
    return lo < s.n_groups && s.groups[lo] == g ? lo : -1;
}

// LDS of mot_clear_kernel, dynamic (65 KiB: above the 64 KiB a kernel gets without the opt-in)
struct ClearLds {
    HungLds<MYDET_EVAL_MAX_GT> h;                // MYDET_EVAL_MAX_GT == MYDET_EVAL_MAX_DT
    int32_t last[MYDET_MOT_MAX_IDS];             // per ground-truth identity: the hypothesis identity of its latest match
    int32_t present[MYDET_MOT_MAX_IDS], matched[MYDET_MOT_MAX_IDS];
    int32_t col_of_id[MYDET_MOT_MAX_IDS];        // per hypothesis identity: its column in the frame, or -1
    int32_t row_match[MYDET_EVAL_MAX_GT];        // the column of a row, or -1
    int32_t col_row[MYDET_EVAL_MAX_DT];          // keep pass: the lowest row that claims a column
    int32_t rem_rows[MYDET_EVAL_MAX_GT], rem_cols[MYDET_EVAL_MAX_DT];
    unsigned char flags[MYDET_MOT_MAX_IDS];      // bit 0: ever matched; bit 1: matched in its previous present frame
};
static_assert(MYDET_EVAL_MAX_GT == MYDET_EVAL_MAX_DT, "one HungLds serves both orientations");

struct ClearCost {
    const double *iou;                           // the group's block: [column (hypothesis)][row (ground truth)]
    const int32_t *rem_rows, *rem_cols;
    int ng;
    bool transposed;                             // the routine's rows are the remaining columns
    double thr;
    __device__ __forceinline__ int64_t operator()(int i, int j) const {
        const int r = rem_rows[transposed ? j : i], c = rem_cols[transposed ? i : j];
        const double v = iou[(int64_t)c * ng + r];
        return v >= thr ? MOT_ONE - (int64_t)floor(v * 65536.0) : MOT_BIG;
    }
};

__global__ __launch_bounds__(MOT_WAVE) void mot_clear_kernel(const mydet_eval_set s, const mydet_mot_set m, const MotThresholds q,
                                                             const double *ious, int64_t *counts, double *siou_out, int32_t *present,
                                                             int32_t *matched, int32_t *gt_match) {
    extern __shared__ __align__(16) unsigned char mot_raw[];
    ClearLds &L = *reinterpret_cast<ClearLds *>(mot_raw);
    const int lane = threadIdx.x;
    const int u = blockIdx.x / q.T, t = blockIdx.x - u * q.T;
    const int k = u / m.S, sq = u - k * m.S;
    const double thr = q.iou[t];
    const int id0 = m.gt_id_start[u], n_gid = m.gt_id_start[u + 1] - id0, n_hid = m.dt_id_start[u + 1] - m.dt_id_start[u];
    if (n_gid < 0 || n_gid > MYDET_MOT_MAX_IDS || n_hid < 0 || n_hid > MYDET_MOT_MAX_IDS) return;     // tables that disagree
    for (int o = lane; o < n_gid; o += MOT_WAVE) {
        L.last[o] = -1;
        L.present[o] = 0;
        L.matched[o] = 0;
        L.flags[o] = 0;
    }
    for (int h = lane; h < n_hid; h += MOT_WAVE) L.col_of_id[h] = -1;
    __syncthreads();
    const uint64_t before = (1ull << lane) - 1;
    int64_t tp = 0, fp = 0, fn = 0, idsw = 0, frag = 0;
    double siou = 0.0;
    const int f_end = min(m.seq_start[sq + 1], s.I);
    for (int f = max(m.seq_start[sq], 0); f < f_end; ++f) {
        const int g = k * s.I + f;
        const int d0 = s.dt_start[g], nd = s.dt_start[g + 1] - d0, g0 = s.gt_start[g], ng = s.gt_start[g + 1] - g0;
        if (nd < 0 || ng < 0 || nd > MYDET_EVAL_MAX_DT || ng > MYDET_EVAL_MAX_GT) continue;
        const int c = nd > 0 && ng > 0 ? mot_listed(s, g) : -1;
        if (nd > 0 && ng > 0 && c < 0) continue;
        const double *iou = c >= 0 ? ious + s.pair_start[c] : ious;
        for (int r = lane; r < ng; r += MOT_WAVE) L.row_match[r] = -1;
        for (int j = lane; j < nd; j += MOT_WAVE) {
            L.col_row[j] = 0x7fffffff;
            const int h = m.dt_id[d0 + j];
            if ((unsigned)h < (unsigned)n_hid) L.col_of_id[h] = j;
        }
        __syncthreads();
        // 1. keep: a row claims the column of its last identity; of two rows with one last the lower wins
        if (nd > 0) {
            for (int r = lane; r < ng; r += MOT_WAVE) {
                const int o = m.gt_id[g0 + r];
                const int l = (unsigned)o < (unsigned)n_gid ? L.last[o] : -1;
                const int j = (unsigned)l < (unsigned)n_hid ? L.col_of_id[l] : -1;
                if (j >= 0 && iou[(int64_t)j * ng + r] >= thr) {
                    L.row_match[r] = j;
                    atomicMin(&L.col_row[j], r);
                }
            }
            __syncthreads();
            for (int r = lane; r < ng; r += MOT_WAVE) {
                const int j = L.row_match[r];
                if (j >= 0 && L.col_row[j] != r) L.row_match[r] = -1;
            }
            __syncthreads();
        }
        // 2. assign the rest, relative order kept
        int nr = 0, nc = 0;
        for (int b = 0; b < ng; b += MOT_WAVE) {
            const int r = b + lane;
            const bool left = r < ng && L.row_match[r] < 0;
            const uint64_t bal = __ballot(left);
            if (left) L.rem_rows[nr + __popcll(bal & before)] = r;
            nr += __popcll(bal);
        }
        for (int b = 0; b < nd; b += MOT_WAVE) {
            const int j = b + lane;
            const bool left = j < nd && L.col_row[j] == 0x7fffffff;
            const uint64_t bal = __ballot(left);
            if (left) L.rem_cols[nc + __popcll(bal & before)] = j;
            nc += __popcll(bal);
        }
        __syncthreads();
        if (nr > 0 && nc > 0) {
            ClearCost cost = {iou, L.rem_rows, L.rem_cols, ng, nr > nc, thr};
            const int hn = nr > nc ? nc : nr, hm = nr > nc ? nr : nc;
            hung_solve(L.h, hn, hm, cost, lane);
            for (int j = lane; j < hm; j += MOT_WAVE) {
                const int i = L.h.p[j];
                if (i < 0) continue;
                const int r = L.rem_rows[cost.transposed ? j : i], cc = L.rem_cols[cost.transposed ? i : j];
                if (iou[(int64_t)cc * ng + r] >= thr) L.row_match[r] = cc;
            }
            __syncthreads();
        }
        // 3 and 4. count, rows ascending
        int n_match = 0;
        for (int b = 0; b < ng; b += MOT_WAVE) {
            const int r = b + lane;
            const int j = r < ng ? L.row_match[r] : -1;
            const int o = r < ng ? m.gt_id[g0 + r] : -1;
            const bool known = (unsigned)o < (unsigned)n_gid;
            const bool hit = j >= 0;
            const double v = hit ? iou[(int64_t)j * ng + r] : 0.0;
            bool sw = false, fr = false;
            if (known) {
                const unsigned fl = L.flags[o];
                if (hit) {
                    const int h = m.dt_id[d0 + j], l = L.last[o];
                    sw = l >= 0 && l != h;
                    fr = (fl & 1u) && !(fl & 2u);
                    L.last[o] = h;
                    L.matched[o] += 1;
                    L.flags[o] = 3;
                } else {
                    L.flags[o] = (unsigned char)(fl & 1u);
                }
                L.present[o] += 1;
            }
            if (gt_match && r < ng) gt_match[(int64_t)t * s.G + g0 + r] = hit ? d0 + j : -1;
            uint64_t bal = __ballot(hit);
            n_match += __popcll(bal);
            idsw += __popcll(__ballot(sw));
            frag += __popcll(__ballot(fr));
            while (bal) {                                              // SIOU: one addition per match, in row order
                const int src = __ffsll((unsigned long long)bal) - 1;
                siou += __shfl(v, src);
                bal &= bal - 1;
            }
        }
        tp += n_match;
        fn += ng - n_match;
        fp += nd - n_match;
        for (int j = lane; j < nd; j += MOT_WAVE) {
            const int h = m.dt_id[d0 + j];
            if ((unsigned)h < (unsigned)n_hid) L.col_of_id[h] = -1;
        }
        __syncthreads();
    }
    for (int o = lane; o < n_gid; o += MOT_WAVE) {
        matched[(int64_t)t * m.n_gt_ids + id0 + o] = L.matched[o];
        if (t == 0) present[id0 + o] = L.present[o];
    }
    if (lane == 0) {
        int64_t *out = counts + ((int64_t)u * q.T + t) * 5;
        out[0] = tp; out[1] = fp; out[2] = fn; out[3] = idsw; out[4] = frag;
        siou_out[(int64_t)u * q.T + t] = siou;
    }
}

// One thread per IoU pair, as in mydet_eval_ious_f64: the pair's unit and identities, then one atomic add per threshold at which
// the pair is eligible.
__global__ __launch_bounds__(256) void mot_overlap_kernel(const mydet_eval_set s, const mydet_mot_set m, const MotThresholds q,
                                                          const double *ious, int32_t *n) {
    for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < s.n_pairs; p += (int64_t)gridDim.x * 256) {
        int lo = 0, hi = s.n_groups;
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (s.pair_start[mid] <= p) lo = mid; else hi = mid;
        }
        const int g = s.groups[lo];
        const int d0 = s.dt_start[g], nd = s.dt_start[g + 1] - d0, g0 = s.gt_start[g], ng = s.gt_start[g + 1] - g0;
        const int64_t local = p - s.pair_start[lo];
        if (ng <= 0 || local >= (int64_t)nd * ng) continue;
        const int d = (int)(local / ng), j = (int)(local - (int64_t)d * ng);
        const int k = g / s.I, f = g - k * s.I;
        int a = 0, b = m.S;                                            // the sequence of frame f: the last with seq_start <= f
        while (b - a > 1) {
            const int mid = (a + b) >> 1;
            if (m.seq_start[mid] <= f) a = mid; else b = mid;
        }
        const int u = k * m.S + a;
        const int n_gid = m.gt_id_start[u + 1] - m.gt_id_start[u], n_hid = m.dt_id_start[u + 1] - m.dt_id_start[u];
        const int o = m.gt_id[g0 + j], h = m.dt_id[d0 + d];
        if ((unsigned)o >= (unsigned)n_gid || (unsigned)h >= (unsigned)n_hid) continue;
        const int64_t at = m.ov_start[u] + (int64_t)o * n_hid + h;
        if (at >= m.n_ov) continue;
        const double v = ious[p];
        for (int t = 0; t < q.T; ++t)
            if (v >= q.iou[t]) atomicAdd(n + (int64_t)t * m.n_ov + at, 1);
    }
}

struct IdCost {
    const int32_t *n;                            // [ground-truth identity][hypothesis identity]
    int n_hid;
    bool transposed;                             // the routine's rows are the hypothesis identities
    int64_t frames;
    __device__ __forceinline__ int64_t operator()(int i, int j) const {
        return frames - n[transposed ? (int64_t)j * n_hid + i : (int64_t)i * n_hid + j];
    }
};

__global__ __launch_bounds__(MOT_WAVE) void mot_id_assign_kernel(const mydet_mot_set m, int T, const int32_t *n, int64_t *idtp) {
    extern __shared__ __align__(16) unsigned char mot_raw[];
    HungLds<MYDET_MOT_MAX_IDS> &L = *reinterpret_cast<HungLds<MYDET_MOT_MAX_IDS> *>(mot_raw);
    const int lane = threadIdx.x;
    const int u = blockIdx.x / T, t = blockIdx.x - u * T;
    const int n_gid = m.gt_id_start[u + 1] - m.gt_id_start[u], n_hid = m.dt_id_start[u + 1] - m.dt_id_start[u];
    if (n_gid < 0 || n_gid > MYDET_MOT_MAX_IDS || n_hid < 0 || n_hid > MYDET_MOT_MAX_IDS) return;
    int64_t sum = 0;
    if (n_gid > 0 && n_hid > 0 && m.ov_start[u] + (int64_t)n_gid * n_hid <= m.n_ov) {
        const int sq = u % m.S;
        IdCost cost = {n + (int64_t)t * m.n_ov + m.ov_start[u], n_hid, n_gid > n_hid, (int64_t)(m.seq_start[sq + 1] - m.seq_start[sq])};
        const int hn = cost.transposed ? n_hid : n_gid, hm = cost.transposed ? n_gid : n_hid;
        hung_solve(L, hn, hm, cost, lane);
        for (int j = lane; j < hm; j += MOT_WAVE)
            if (L.p[j] >= 0) sum += cost.frames - cost(L.p[j], j);
        sum = wave_sum(sum);
    }
    if (lane == 0) idtp[(int64_t)u * T + t] = sum;
}

int mot_thresholds(MotThresholds &q, const double *iou_thrs, int T) {
    if (!iou_thrs || T < 1) return MYDET_E_BADARG;
    if (T > MYDET_EVAL_MAX_THRS) return MYDET_E_UNSUPP;
    for (int t = 0; t < T; ++t) {
        if (iou_thrs[t] != iou_thrs[t]) return MYDET_E_BADARG;
        q.iou[t] = iou_thrs[t];
    }
    q.T = T;
    return 0;
}

}  // namespace

extern "C" int mydet_mot_clear_f64(const mydet_eval_set *set, const mydet_mot_set *mot, const double *ious, const double *iou_thrs, int T,
                                   int64_t *counts, double *siou, int32_t *present, int32_t *matched, int32_t *gt_match, void *stream) {
    const int code = mot_check(set, mot);
    if (code) return code;
    MotThresholds q = {};
    const int bad = mot_thresholds(q, iou_thrs, T);
    if (bad) return bad;
    if (!counts || !siou || (set->n_pairs > 0 && !ious) || (mot->n_gt_ids > 0 && (!present || !matched))) return MYDET_E_BADARG;
    const int64_t blocks = (int64_t)mot->S * set->K * T;
    if (blocks > 0x7fffffff) return MYDET_E_UNSUPP;
    static unsigned long long opted = 0ull;
    const int st = mydet_lds_opt_in(opted, mot_clear_kernel, (int)sizeof(ClearLds));
    if (st) return st;
    hipLaunchKernelGGL(mot_clear_kernel, dim3((unsigned)blocks), dim3(MOT_WAVE), sizeof(ClearLds), (hipStream_t)stream, *set, *mot, q, ious,
                       counts, siou, present, matched, gt_match);
    return mydet_launch_status();
}

extern "C" int64_t mydet_mot_scratch_bytes(const mydet_mot_set *mot, int T) {
    if (!mot || mot->n_ov < 0 || T < 1 || T > MYDET_EVAL_MAX_THRS) return 0;
    return mot->n_ov * T * (int64_t)sizeof(int32_t);
}

extern "C" int mydet_mot_id_overlap(const mydet_eval_set *set, const mydet_mot_set *mot, const double *ious, const double *iou_thrs, int T,
                                    void *scratch, int64_t scratch_bytes, void *stream) {
    const int code = mot_check(set, mot);
    if (code) return code;
    MotThresholds q = {};
    const int bad = mot_thresholds(q, iou_thrs, T);
    if (bad) return bad;
    const int64_t need = mydet_mot_scratch_bytes(mot, T);
    if (scratch_bytes < need || (need > 0 && !scratch) || (set->n_pairs > 0 && !ious)) return MYDET_E_BADARG;
    if (need == 0) return 0;
    if (hipMemsetAsync(scratch, 0, (size_t)need, (hipStream_t)stream) != hipSuccess) return mydet_launch_status();
    if (set->n_pairs == 0) return 0;
    int64_t blocks = (set->n_pairs + 255) / 256;
    if (blocks > 256 * 16) blocks = 256 * 16;
    hipLaunchKernelGGL(mot_overlap_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, *set, *mot, q, ious,
                       static_cast<int32_t *>(scratch));
    return mydet_launch_status();
}

extern "C" int mydet_mot_id_assign(const mydet_eval_set *set, const mydet_mot_set *mot, int T, const void *scratch, int64_t scratch_bytes,
                                   int64_t *idtp, void *stream) {
    const int code = mot_check(set, mot);
    if (code) return code;
    if (T < 1) return MYDET_E_BADARG;
    if (T > MYDET_EVAL_MAX_THRS) return MYDET_E_UNSUPP;
    const int64_t need = mydet_mot_scratch_bytes(mot, T);
    if (!idtp || scratch_bytes < need || (need > 0 && !scratch)) return MYDET_E_BADARG;
    const int64_t blocks = (int64_t)mot->S * set->K * T;
    if (blocks > 0x7fffffff) return MYDET_E_UNSUPP;
    hipLaunchKernelGGL(mot_id_assign_kernel, dim3((unsigned)blocks), dim3(MOT_WAVE), sizeof(HungLds<MYDET_MOT_MAX_IDS>), (hipStream_t)stream,
                       *mot, T, static_cast<const int32_t *>(scratch), idtp);
    return mydet_launch_status();
}
