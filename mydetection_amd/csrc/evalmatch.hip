// Detection scoring on the device: COCO's bbox evaluation (useCats = 1) in three stream-ordered launches over the packed arrays
// of include/mydet.h (mydet_eval_set, where the rules are; DESIGN.md section 4 has them too).  Replaces the reference's
// utils/evaluation/coco.py and cepdof.py, which sit on pycocotools: computeIoU, evaluateImg and accumulate.
//   mydet_eval_ious_f64        one thread per (dt, gt) pair of every non-empty group
//   mydet_eval_match_f64       one wavefront per group, one lane per (area range, IoU threshold) problem
//   mydet_eval_accumulate_f64  one wavefront per (category, area range, maxDets, IoU threshold)
// Built with -ffp-contract=off: the float64 IoU is products, sums and ONE division in the documented order, and every recall and
// precision value is one IEEE division of two exactly converted integers.  Counts are integers, formed from ballots and
// population counts, so no scan order can change a bit.  Nothing here uses scratch memory: the per-lane state of the matcher
// (which ground truths a problem has used) is a bit set in LDS, column `lane` of a [word][64] array -- a lane touches only its
// own column (no barrier) and lanes l, l + 32 share a bank without conflict.
#include "common.h"
#include "eval_set.h"
#include "rot_iou.h"

namespace {

constexpr int EV_WAVE = 64;
constexpr int EV_WORDS = MYDET_EVAL_MAX_GT / 32;

struct EvalThresholds {                          // host arrays, copied into the launch
    double iou[MYDET_EVAL_MAX_THRS];
    double lo[MYDET_EVAL_MAX_AREAS], hi[MYDET_EVAL_MAX_AREAS];
    int T, A;
};

struct EvalCurve {
    double rec[MYDET_EVAL_MAX_RECS];
    int max_det[MYDET_EVAL_MAX_DETS];
    int M, R;
};

__device__ __forceinline__ bool eval_gt_ignored(unsigned flags, double area, double lo, double hi) {
    return (flags & MYDET_EVAL_GT_IGNORE) != 0 || area < lo || area > hi;
}

__global__ __launch_bounds__(256) void eval_ious_kernel(const mydet_eval_set s, int64_t n_pairs, double *out) {
    for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < n_pairs; p += (int64_t)gridDim.x * 256) {
        // the listed group that holds pair p: the last c with pair_start[c] <= p (a group without pairs is never that one)
        int lo = 0, hi = s.n_groups;
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (s.pair_start[mid] <= p) lo = mid; else hi = mid;
        }
        const int g = s.groups[lo];
        const int d0 = s.dt_start[g], nd = s.dt_start[g + 1] - d0, g0 = s.gt_start[g], ng = s.gt_start[g + 1] - g0;
        const int64_t local = p - s.pair_start[lo];
        if (ng <= 0 || local >= (int64_t)nd * ng) continue;            // tables that disagree: the pair is not written
        const int d = (int)(local / ng), j = (int)(local - (int64_t)d * ng);
        double iou = 0.0;
        if (s.rotated) {
            const float *a = static_cast<const float *>(s.dt_box) + (int64_t)(d0 + d) * 5;
            const float *b = static_cast<const float *>(s.gt_box) + (int64_t)(g0 + j) * 5;
            iou = (double)rotiou::rot_iou(rotiou::make_box(a[0], a[1], a[2], a[3], a[4]), rotiou::make_box(b[0], b[1], b[2], b[3], b[4]));
        } else {
            const double *a = static_cast<const double *>(s.dt_box) + (int64_t)(d0 + d) * 4;
            const double *b = static_cast<const double *>(s.gt_box) + (int64_t)(g0 + j) * 4;
            const double da = a[2] * a[3], ga = b[2] * b[3];
            const double w = fmin(a[0] + a[2], b[0] + b[2]) - fmax(a[0], b[0]);
            const double h = fmin(a[1] + a[3], b[1] + b[3]) - fmax(a[1], b[1]);
            if (!(w <= 0.0) && !(h <= 0.0)) {
                const double i = w * h;
                const double u = (s.gt_flags[g0 + j] & MYDET_EVAL_GT_CROWD) ? da : da + ga - i;
                iou = i / u;
            }
        }
        out[p] = iou;
    }
}

// One wavefront per listed group.  The A*T problems are laid over the lanes area range by area range: 64 / T ranges per pass,
// lane = la*T + t, so the masks over t of one range are one field of a ballot.  Every loop bound is wave-uniform.
__global__ __launch_bounds__(EV_WAVE) void eval_match_kernel(const mydet_eval_set s, const EvalThresholds q, const double *ious,
                                                             uint32_t *dt_matched, uint32_t *dt_ignored, int32_t *dt_gt) {
    __shared__ uint32_t used[EV_WORDS * EV_WAVE];
    const int c = blockIdx.x, lane = threadIdx.x;
    const int g = s.groups[c];
    const int d0 = s.dt_start[g], nd = s.dt_start[g + 1] - d0, g0 = s.gt_start[g], ng = s.gt_start[g + 1] - g0;
    if (nd <= 0 || ng < 0 || ng > MYDET_EVAL_MAX_GT) return;
    const double *iou = ious + s.pair_start[c];
    const int per_pass = EV_WAVE / q.T;
    const int words = (ng + 31) >> 5;
    const int la = lane / q.T, t = lane - la * q.T;
    const uint64_t field = (1ull << q.T) - 1;                          // T <= 32
    for (int a0 = 0; a0 < q.A; a0 += per_pass) {
        const int a = a0 + la;
        const bool live = la < per_pass && a < q.A;
        const double lo = q.lo[live ? a : 0], hi = q.hi[live ? a : 0];
        const double thr = fmin(q.iou[t], 1.0 - 1e-10);
        for (int w = 0; w < words; ++w) used[w * EV_WAVE + lane] = 0;
        for (int d = 0; d < nd; ++d) {
            const double *row = iou + (int64_t)d * ng;
            double best = thr;
            int m = -1, m_ignored = 0;
            // ground truths in (gtIg ascending, annotation order) order: those with gtIg == 0, then, for a problem that has found
            // none of them, those with gtIg == 1
            for (int pass = 0; pass < 2; ++pass) {
                const bool walk = live && m < 0;                       // pass 1: a match from pass 0 ends the walk
                if (!__any(walk)) break;
                for (int j = 0; j < ng; ++j) {
                    const unsigned fl = s.gt_flags[g0 + j];
                    const int ig = eval_gt_ignored(fl, s.gt_area[g0 + j], lo, hi) ? 1 : 0;
                    const bool taken = ((used[(j >> 5) * EV_WAVE + lane] >> (j & 31)) & 1u) != 0 && !(fl & MYDET_EVAL_GT_CROWD);
                    const double v = row[j];
                    if (walk && ig == pass && !taken && !(v < best)) {
                        best = v;
                        m = j;
                        m_ignored = pass;
                    }
                }
            }
            const bool matched = live && m >= 0;
            if (matched) used[(m >> 5) * EV_WAVE + lane] |= 1u << (m & 31);
            const double area = s.dt_area[d0 + d];
            const bool ignored = live && (matched ? m_ignored != 0 : (area < lo || area > hi));
            const uint64_t bm = __ballot(matched), bi = __ballot(ignored);
            if (lane < per_pass && a0 + lane < q.A) {
                const int64_t o = (int64_t)(a0 + lane) * s.D + d0 + d;
                dt_matched[o] = (uint32_t)((bm >> (lane * q.T)) & field);
                dt_ignored[o] = (uint32_t)((bi >> (lane * q.T)) & field);
            }
            if (dt_gt && live) dt_gt[((int64_t)a * q.T + t) * s.D + d0 + d] = matched ? g0 + m : -1;
        }
    }
}

// The state of EV_DEPTH chunks of 64 positions from `base` of a category's order: bit EV_KEPT rank < maxDets, EV_TP matched and
// not ignored, EV_FP neither; 0 beyond n.  The chunks' gathers (order, then rank and the two masks) are independent, so a
// wavefront has EV_DEPTH times as many loads in flight as one chunk gives it: the launch is bound by their latency.
constexpr int EV_DEPTH = 4;
constexpr unsigned EV_KEPT = 1, EV_TP = 2, EV_FP = 4;

__device__ __forceinline__ void eval_fetch(const int32_t *order, int n, int base, int lane, const int32_t *dt_rank, const uint32_t *mrow,
                                           const uint32_t *irow, int max_det, int t, int (&e)[EV_DEPTH], unsigned (&st)[EV_DEPTH]) {
#pragma unroll
    for (int u = 0; u < EV_DEPTH; ++u) {
        const int i = base + u * EV_WAVE + lane;
        e[u] = i < n ? order[i] : -1;
    }
#pragma unroll
    for (int u = 0; u < EV_DEPTH; ++u) {
        st[u] = 0;
        if (e[u] >= 0) {
            const bool keep = dt_rank[e[u]] < max_det;
            const bool mb = (mrow[e[u]] >> t) & 1u, ib = (irow[e[u]] >> t) & 1u;
            st[u] = (keep ? EV_KEPT : 0u) | (keep && mb && !ib ? EV_TP : 0u) | (keep && !mb && !ib ? EV_FP : 0u);
        }
    }
}

// One wavefront per (k, a, m, t), t fastest.  Forward: the totals.  Backward, 64 positions at a time: the counts at a position
// are the totals behind the chunk minus what the chunk's later lanes hold, the precision envelope is a suffix maximum carried
// from chunk to chunk (four chunks are fetched together: eval_fetch), and a position at which the recall passes thresholds writes their entries.
__global__ __launch_bounds__(EV_WAVE) void eval_accumulate_kernel(const mydet_eval_set s, const EvalThresholds q, const EvalCurve cv,
                                                                  const int32_t *order, const int32_t *cat_start, const int32_t *dt_rank,
                                                                  const uint32_t *dt_matched, const uint32_t *dt_ignored,
                                                                  double *precision, double *recall, double *scores) {
    const int lane = threadIdx.x;
    int b = blockIdx.x;
    const int t = b % q.T; b /= q.T;
    const int mi = b % cv.M; b /= cv.M;
    const int a = b % q.A;
    const int k = b / q.A;
    const int R = cv.R;
    const double lo = q.lo[a], hi = q.hi[a];
    const int64_t p0 = (((int64_t)t * R * s.K + k) * q.A + a) * cv.M + mi;      // entry r is at p0 + r * pstep
    const int64_t pstep = (int64_t)s.K * q.A * cv.M;

    const int gs = s.gt_start[(int64_t)k * s.I], ge = s.gt_start[(int64_t)(k + 1) * s.I];
    int npig = 0;
    for (int j0 = gs; j0 < ge; j0 += EV_WAVE) {
        const int j = j0 + lane;
        const bool counts = j < ge && !eval_gt_ignored(s.gt_flags[j < ge ? j : gs], s.gt_area[j < ge ? j : gs], lo, hi);
        npig += __popcll(__ballot(counts));
    }
    if (npig == 0) {
        for (int r = lane; r < R; r += EV_WAVE) {
            precision[p0 + r * pstep] = -1.0;
            scores[p0 + r * pstep] = -1.0;
        }
        if (lane == 0) recall[(((int64_t)t * s.K + k) * q.A + a) * cv.M + mi] = -1.0;
        return;
    }
    const int o0 = cat_start[k], n = cat_start[k + 1] - o0;
    const int max_det = cv.max_det[mi];
    const uint32_t *mrow = dt_matched + (int64_t)a * s.D, *irow = dt_ignored + (int64_t)a * s.D;

    int tp_end = 0, fp_end = 0, kept_end = 0;
    int e[EV_DEPTH];
    unsigned st[EV_DEPTH];
    for (int base = 0; base < n; base += EV_WAVE * EV_DEPTH) {
        eval_fetch(order + o0, n, base, lane, dt_rank, mrow, irow, max_det, t, e, st);
#pragma unroll
        for (int u = 0; u < EV_DEPTH; ++u) {
            tp_end += __popcll(__ballot((st[u] & EV_TP) != 0));
            fp_end += __popcll(__ballot((st[u] & EV_FP) != 0));
            kept_end += __popcll(__ballot((st[u] & EV_KEPT) != 0));
        }
    }
    const double dn = (double)npig;
    const int nd = kept_end, tp_all = tp_end;
    const uint64_t upto = lane == 63 ? ~0ull : (1ull << (lane + 1)) - 1;       // this lane and the ones before it
    double later = 0.0;                                                        // max precision behind the chunk; precision >= 0
    constexpr int STEP = EV_WAVE * EV_DEPTH;
    for (int base = n > 0 ? ((n - 1) / STEP) * STEP : -1; base >= 0; base -= STEP) {
        eval_fetch(order + o0, n, base, lane, dt_rank, mrow, irow, max_det, t, e, st);
#pragma unroll
        for (int u = EV_DEPTH - 1; u >= 0; --u) {                              // a chunk beyond n holds nothing and changes nothing
            const bool keep = (st[u] & EV_KEPT) != 0, tp = (st[u] & EV_TP) != 0, fp = (st[u] & EV_FP) != 0;
            const uint64_t bt = __ballot(tp), bf = __ballot(fp), bk = __ballot(keep);
            const int tpi = tp_end - __popcll(bt) + __popcll(bt & upto);
            const int fpi = fp_end - __popcll(bf) + __popcll(bf & upto);
            const int pos = kept_end - __popcll(bk) + __popcll(bk & upto) - 1; // index among the kept detections
            double env = keep ? (double)tpi / ((double)(fpi + tpi) + 2.220446049250313e-16) : 0.0;
#pragma unroll
            for (int off = 1; off < EV_WAVE; off <<= 1) {
                const double o = __shfl_down(env, off);
                if (lane + off < EV_WAVE) env = fmax(env, o);
            }
            env = fmax(env, later);
            later = __shfl(env, 0);
            if (keep && (pos == 0 || tp)) {
                const double rc = (double)tpi / dn;
                int r = 0;
                if (pos != 0) {                                                // the first threshold above the recall before it
                    const double before = (double)(tpi - 1) / dn;
                    int rl = 0, rh = R;
                    while (rl < rh) {
                        const int mid = (rl + rh) >> 1;
                        if (cv.rec[mid] > before) rh = mid; else rl = mid + 1;
                    }
                    r = rl;
                }
                const double sc = s.dt_score[e[u]];
                for (; r < R && cv.rec[r] <= rc; ++r) {
                    precision[p0 + r * pstep] = env;
                    scores[p0 + r * pstep] = sc;
                }
            }
            tp_end -= __popcll(bt);
            fp_end -= __popcll(bf);
            kept_end -= __popcll(bk);
        }
    }
    const double rc_last = (double)tp_all / dn;
    for (int r = lane; r < R; r += EV_WAVE)
        if (nd == 0 || cv.rec[r] > rc_last) {
            precision[p0 + r * pstep] = 0.0;
            scores[p0 + r * pstep] = 0.0;
        }
    if (lane == 0) recall[(((int64_t)t * s.K + k) * q.A + a) * cv.M + mi] = nd ? rc_last : 0.0;
}

int eval_thresholds(EvalThresholds &q, const double *iou_thrs, int T, const double *area_rng, int A) {
    if (!iou_thrs || !area_rng || T < 1 || A < 1) return MYDET_E_BADARG;
    if (T > MYDET_EVAL_MAX_THRS || A > MYDET_EVAL_MAX_AREAS) return MYDET_E_UNSUPP;
    for (int t = 0; t < T; ++t) {
        if (iou_thrs[t] != iou_thrs[t]) return MYDET_E_BADARG;
        q.iou[t] = iou_thrs[t];
    }
    for (int a = 0; a < A; ++a) {
        q.lo[a] = area_rng[2 * a];
        q.hi[a] = area_rng[2 * a + 1];
        if (!(q.lo[a] <= q.hi[a])) return MYDET_E_BADARG;                      // NaN too
    }
    q.T = T; q.A = A;
    return 0;
}

}  // namespace

extern "C" int mydet_eval_ious_f64(const mydet_eval_set *set, double *ious, void *stream) {
    const int code = eval_check_set(set);
    if (code) return code;
    if (set->n_pairs == 0) return 0;
    if (!ious) return MYDET_E_BADARG;
    int64_t blocks = (set->n_pairs + 255) / 256;
    if (blocks > 256 * 16) blocks = 256 * 16;
    hipLaunchKernelGGL(eval_ious_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, *set, set->n_pairs, ious);
    return mydet_launch_status();
}

extern "C" int mydet_eval_match_f64(const mydet_eval_set *set, const double *ious, const double *iou_thrs, int T, const double *area_rng,
                                    int A, uint32_t *dt_matched, uint32_t *dt_ignored, int32_t *dt_gt, void *stream) {
    const int code = eval_check_set(set);
    if (code) return code;
    EvalThresholds q = {};
    const int bad = eval_thresholds(q, iou_thrs, T, area_rng, A);
    if (bad) return bad;
    if (set->D == 0) return 0;
    if (!dt_matched || !dt_ignored || (set->n_pairs > 0 && !ious)) return MYDET_E_BADARG;
    hipLaunchKernelGGL(eval_match_kernel, dim3((unsigned)set->n_groups), dim3(EV_WAVE), 0, (hipStream_t)stream, *set, q, ious, dt_matched,
                       dt_ignored, dt_gt);
    return mydet_launch_status();
}

extern "C" int mydet_eval_accumulate_f64(const mydet_eval_set *set, const int32_t *order, const int32_t *cat_start, const int32_t *dt_rank,
                                         const uint32_t *dt_matched, const uint32_t *dt_ignored, int T, const double *area_rng, int A,
                                         const int32_t *max_dets, int M, const double *rec_thrs, int R, double *precision,
                                         double *recall, double *scores, void *stream) {
    const int code = eval_check_set(set);
    if (code) return code;
    if (T < 1 || A < 1 || M < 1 || R < 1 || !area_rng || !max_dets || !rec_thrs) return MYDET_E_BADARG;
    if (T > MYDET_EVAL_MAX_THRS || A > MYDET_EVAL_MAX_AREAS || M > MYDET_EVAL_MAX_DETS || R > MYDET_EVAL_MAX_RECS) return MYDET_E_UNSUPP;
    EvalThresholds q = {};
    EvalCurve cv = {};
    const double zero = 0.0;
    const int bad = eval_thresholds(q, &zero, 1, area_rng, A);
    if (bad) return bad;
    q.T = T;
    for (int m = 0; m < M; ++m) {
        if (max_dets[m] < 1 || (m > 0 && max_dets[m] < max_dets[m - 1])) return MYDET_E_BADARG;
        cv.max_det[m] = max_dets[m];
    }
    for (int r = 0; r < R; ++r) {
        if (rec_thrs[r] != rec_thrs[r] || (r > 0 && rec_thrs[r] < rec_thrs[r - 1])) return MYDET_E_BADARG;
        cv.rec[r] = rec_thrs[r];
    }
    if (max_dets[M - 1] > MYDET_EVAL_MAX_DT) return MYDET_E_UNSUPP;
    cv.M = M; cv.R = R;
    if (!cat_start || !precision || !recall || !scores) return MYDET_E_BADARG;
    if (set->D > 0 && (!order || !dt_rank || !dt_matched || !dt_ignored)) return MYDET_E_BADARG;
    const int64_t blocks = (int64_t)set->K * A * M * T;
    if (blocks > 0x7fffffff) return MYDET_E_UNSUPP;
    hipLaunchKernelGGL(eval_accumulate_kernel, dim3((unsigned)blocks), dim3(EV_WAVE), 0, (hipStream_t)stream, *set, q, cv, order, cat_start,
                       dt_rank, dt_matched, dt_ignored, precision, recall, scores);
    return mydet_launch_status();
}
