// Multi-object tracking on the device: detection records of consecutive frames -> persistent identities and Kalman-filtered
// boxes, without a per-frame copy of the records to the host.
//
// State model: the reference's KFTracklet (utils/structures.py:445-529) over RotBBoxKalmanFilter (utils/kalman_filter.py:77-142):
// a constant-velocity Kalman filter on (cx, cy, w, h, angle).  F couples parameter i only with its own velocity, H selects the five
// parameters and P0, Q, R are diagonal (the area scaling multiplies whole rows of diagonal matrices), so the 10 x 10 covariance
// is five independent symmetric 2 x 2 blocks (pxx, pxv, pvv) for ever and the 5 x 5 inverse of the update is five reciprocals.
// The reference ships no loop around that model; the association rules are this project's (include/mydet.h).
//
// One workgroup per stream, thread = track slot: a track lives in its thread's registers for all F frames of the launch and
// only the frame's detections go through LDS.  Per frame:
//   1. stage the <= 512 detections of the record in LDS with their pair-test planes (corners + area, or the rotiou::Box of
//      rot_iou.h) and rank them by (score descending, record slot ascending);
//   2. predict every live track;
//   3. greedy association: the walk over the ranked detections is sequential, its body is lane-per-track -- every thread
//      computes the IoU of its own predicted box with the detection, a 64-bit key (IoU bits, ~slot) is maximised over the wave
//      by shuffles and over the waves through LDS: one barrier per detection.  With score bands (mydet_track_assoc) the same
//      walk is stage 1 and then stage 2, because every high detection is ranked before every low one: only the threshold and
//      the track's eligibility change at the boundary.  The optimal assignment instead publishes every predicted track's side
//      of the pair test in LDS and lets wavefront 0 run hung_solve (hung.h) once per stage, the costs formed on the fly;
//   4. matched tracks take the Kalman update; 5. infeasible and long-missed tracks are retired; 6. the unmatched detections
//      above new_thres are born into the lowest free slots -- ranks by ballot and popcount, no serial loop.
// Built with -ffp-contract=off: the float32 operation order below IS the definition (tests/_track_ref.py restates it in numpy
// and is held to the reference's float64 on tests/golden/kf_tracklet.npz).
#include <type_traits>

#include "common.h"
#include "hung.h"
#include "rot_iou.h"

namespace {

constexpr int KMAX = MYDET_REC_TOPK;
constexpr int TMAX = MYDET_TRACK_MAX_TRACKS;
constexpr int NWMAX = TMAX / 64;
// the instances of track_kernel: today's walk, the walk with score bands, the optimal assignment (bands a launch argument)
constexpr int ASSOC_GREEDY = 0, ASSOC_GREEDY_BANDS = 1, ASSOC_OPTIMAL = 2;
constexpr int64_t ASSOC_INELIGIBLE = 2 * MOT_ONE;

struct TrackArgs {
    const int32_t *rec;               // record of frame f of stream s at rec + s*stream_st + f*frame_st (words)
    int64_t stream_st, frame_st;
    int F, MT;
    mydet_track_params p;
    int32_t *state;
    int64_t state_words;              // per stream
    float *obox, *oscore;
    int64_t *ocls, *oid;
    int32_t *omissed, *ocount, *odropped;
    mydet_track_assoc as;             // read by the instances with bands or the optimal assignment only
    const int32_t *shift;             // null, or the camera motion of frame o at shift + 4 o: (dx, dy, valid, n_valid)
    const int32_t *warp;              // null, or its similarity model at warp + 8 o: (a, b, tx, ty, s_q, deg_q, valid, n_inliers); never with shift
};
// The arguments of the instances with an appearance (mydet_track_frames_appear_f32): the others keep TrackArgs as it was
struct TrackAppearArgs : TrackArgs {
    mydet_track_appear ap;
    const uint16_t *desc;             // the descriptors of frame o at desc + o * KMAX * 128, row = record slot
    int32_t *astate;                  // per stream: has [MT], then tmpl [128][MT] (bin-major: the lanes of a wave read adjacent words)
    int64_t astate_words;
    int32_t *osim, *ohow;
#ifdef MYDET_TRACK_APPEAR_OPTIMAL                                     // mydet_track_frames_appear_optimal_f32 only
    int32_t *sim_ws;                  // per stream: S(j, d) at sim_ws[d * MT + j], KMAX * MT words
    int weight;                       // 0..256: the share of the appearance in the fused affinity
#endif
};
template <bool APPEAR>
using TrackKernelArgs = std::conditional_t<APPEAR, TrackAppearArgs, TrackArgs>;
constexpr int ABINS = MYDET_APPEAR_BINS;

// LDS of the optimal assignment, dynamic: with the kernel's static arrays it is above the 64 KiB a kernel gets without the opt-in
struct AssocLds {
    HungLds<TMAX + KMAX> h;           // columns: the track slots, then one dummy per row
    float t[7][TMAX];                 // every track's side of the pair test after predict
    int64_t tcls[TMAX];
    int32_t tmissed[TMAX];            // missed after predict (>= 1), or -1 for a slot that is not live
    int32_t tmd[TMAX];                // the record slot a track took, or -1
    int32_t rowd[KMAX], rowp[KMAX];   // a stage's rows: record slot and rank
};
// The optimal assignment with an appearance publishes `has` too: the similarity phase and the cost read other tracks' flags
struct AssocAppearLds : AssocLds {
    int32_t thas[TMAX];
};
// An upper bound of track_kernel's static arrays (33 - 37 KiB).  The opt-in asks for the dynamic part plus this, so the request
// covers the kernel's whole LDS whether the runtime holds the limit against the dynamic part alone or against the sum.
constexpr int ASSOC_STATIC_LDS = 40 * 1024;

// The cost of (row i, column j) of one stage (include/mydet.h: mydet_track_assoc).  The IoU is the float32 expression of the
// greedy walk, operation for operation.
template <bool ROT>
struct AssocCost {
    const float (*g)[KMAX];           // the detections' pair-test planes
    const int64_t *dcl;
    const AssocLds *A;
    int MT;
    bool second;                      // stage 2: only the tracks matched or born in the previous frame
    float thr;
    __device__ __forceinline__ int64_t operator()(int i, int j) const {
        if (j >= MT) return MOT_ONE;
        const int d = A->rowd[i], tm = A->tmissed[j];
        if (tm < 0 || A->tmd[j] >= 0 || A->tcls[j] != dcl[d] || (second && tm != 1)) return ASSOC_INELIGIBLE;
        float iou;
        if constexpr (ROT) {
            const rotiou::Box bi{g[0][d], g[1][d], g[2][d], g[3][d], g[4][d], g[5][d], g[6][d]};
            const rotiou::Box bj{A->t[0][j], A->t[1][j], A->t[2][j], A->t[3][j], A->t[4][j], A->t[5][j], A->t[6][j]};
            iou = rotiou::rot_iou(bi, bj);
        } else {
            const float xx1 = fmaxf(g[0][d], A->t[0][j]), yy1 = fmaxf(g[1][d], A->t[1][j]);
            const float xx2 = fminf(g[2][d], A->t[2][j]), yy2 = fminf(g[3][d], A->t[3][j]);
            const float ww = fmaxf(0.0f, xx2 - xx1), hh = fmaxf(0.0f, yy2 - yy1);
            const float inter = ww * hh;
            iou = inter / (g[4][d] + A->t[4][j] - inter);
        }
        if (!(iou > thr)) return ASSOC_INELIGIBLE;                 // a NaN (0/0) is never eligible
        return MOT_ONE - (int64_t)(int)floorf(iou * 65536.0f);
    }
};

// The fused cost (include/mydet.h: mydet_track_frames_appear_optimal_f32): AssocCost's, then the gate and the affinity m from ONE
// word of the workspace the similarity phase filled.  An eligible pair of AssocCost is MOT_ONE - q, so q comes back out of it.
template <bool ROT>
struct AssocAppearCost {
    AssocCost<ROT> iou;
    const int32_t *thas;              // has[j] before this frame's update
    const int32_t *ws;                // the stream's S: ws[d * MT + j]
    int gate, weight;
    __device__ __forceinline__ int64_t operator()(int i, int j) const {
        const int64_t c = iou(i, j);
        if (j >= iou.MT || c == ASSOC_INELIGIBLE || !thas[j]) return c;
        const int sv = ws[iou.A->rowd[i] * iou.MT + j];
        if (gate > 0 && sv < gate) return ASSOC_INELIGIBLE;
        const int q = (int)(MOT_ONE - c);
        return MOT_ONE - (int64_t)(((256 - weight) * q + weight * (sv >> 1)) >> 8);
    }
};

__device__ __forceinline__ unsigned sortable(float f) {
    const unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// Python's a % 180 (the sign of the divisor): fmodf is exact, the one rounding is the add
__device__ __forceinline__ float mod180(float a) {
    const float r = fmodf(a, 180.0f);
    if (r == 0.0f) return 0.0f;
    return r < 0.0f ? r + 180.0f : r;
}

__device__ __forceinline__ int prefix_bits(const unsigned long long *mask, int i) {
    int k = 0;
    for (int w = 0; w < (i >> 6); ++w) k += __popcll(mask[w]);
    return k + __popcll(mask[i >> 6] & ((1ull << (i & 63)) - 1ull));
}

__device__ __forceinline__ unsigned long long wave_max(unsigned long long v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const unsigned long long o = __shfl_xor(v, off, 64);
        v = o > v ? o : v;
    }
    return v;
}

// S(j, d) = sum over the bins of min(tmpl[b][j], 256 * desc[d][b]); tm = the track's column of the template, dr = the row
__device__ __forceinline__ int appear_sim(const int32_t *tm, int MT, const uint16_t *dr) {
    int s = 0;
#pragma unroll 4                                                       // 32 template words in flight: the sum is latency-bound
    for (int g = 0; g < ABINS / 8; ++g) {
        const uint4 q = reinterpret_cast<const uint4 *>(dr)[g];
        const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            s += min(tm[(int64_t)(g * 8 + 2 * k) * MT], (int)((w[k] & 0xffffu) << 8));
            s += min(tm[(int64_t)(g * 8 + 2 * k + 1) * MT], (int)((w[k] >> 16) << 8));
        }
    }
    return s;
}

// The similarity phase of the fused cost, on every wave of the workgroup between predict and the solve: S(j, d) of every needed
// pair (include/mydet.h: the workspace of mydet_track_frames_appear_optimal_f32) into ws[d * MT + j].  A wave takes every
// nwave-th detection and walks the track slots 64 at a time: the need test is lane-per-track with the IoU of the walk, operation
// for operation, and a ballot picks the form of the sum.  Dense (>= APPEAR_DENSE lanes need their pair): lanes own tracks, every
// lane sums its own column -- the 64 template words of a bin are adjacent, one load serves the wave.  Sparse: lanes own bins,
// two each, for up to four pairs at a time, and a shuffle tree adds them: one round of loads per four pairs instead of a
// chain of 128.  Both are the same integer sum.
constexpr int APPEAR_DENSE = 16;
template <bool ROT>
__device__ __forceinline__ void appear_sim_phase(const float (*g)[KMAX], const float *sc, const int64_t *dcl, const AssocAppearLds &A, int n,
                                                 int MT, const mydet_track_assoc &as, float match_thres, const int32_t *tmpl,
                                                 const uint16_t *dframe, int32_t *ws, int lane, int wave, int nwave) {
    for (int d0 = wave; d0 < n; d0 += nwave) {
        const int d = __builtin_amdgcn_readfirstlane(d0);
        float thr = match_thres;
        bool second = false;
        if (as.bands) {
            const float s = sc[d];
            if (!(s >= as.high_thres)) {
                if (!(s >= as.low_thres && s < as.high_thres)) continue;      // in no band: no pair of it is needed
                thr = as.low_match_thres;
                second = true;
            }
        }
        const uint16_t *dr = dframe + (int64_t)d * ABINS;
        const int dlo = (int)dr[lane] << 8, dhi = (int)dr[lane + 64] << 8;
        const int64_t dc = dcl[d];
        for (int j0 = 0; j0 < MT; j0 += 64) {
            const int j = j0 + lane;                                   // < blockDim.x: every thread published its slot
            const int tmj = A.tmissed[j];
            bool need = tmj >= 0 && A.thas[j] != 0 && A.tcls[j] == dc && (!second || tmj == 1);
            if (need) {
                float iou;
                if constexpr (ROT) {
                    const rotiou::Box bi{g[0][d], g[1][d], g[2][d], g[3][d], g[4][d], g[5][d], g[6][d]};
                    const rotiou::Box bj{A.t[0][j], A.t[1][j], A.t[2][j], A.t[3][j], A.t[4][j], A.t[5][j], A.t[6][j]};
                    iou = rotiou::rot_iou(bi, bj);
                } else {
                    const float xx1 = fmaxf(g[0][d], A.t[0][j]), yy1 = fmaxf(g[1][d], A.t[1][j]);
                    const float xx2 = fminf(g[2][d], A.t[2][j]), yy2 = fminf(g[3][d], A.t[3][j]);
                    const float ww = fmaxf(0.0f, xx2 - xx1), hh = fmaxf(0.0f, yy2 - yy1);
                    const float inter = ww * hh;
                    iou = inter / (g[4][d] + A.t[4][j] - inter);
                }
                need = iou > thr;                                      // a NaN (0/0) is never needed
            }
            unsigned long long bal = __ballot(need);
            if (__popcll(bal) >= APPEAR_DENSE) {
                if (need) ws[d * MT + j] = appear_sim(tmpl + j, MT, dr);
                continue;
            }
            while (bal) {
                int jj[4], v[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    jj[k] = bal ? j0 + __ffsll((long long)bal) - 1 : -1;
                    bal &= bal - 1ull;                                 // 0 stays 0
                }
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    v[k] = 0;
                    if (jj[k] >= 0) v[k] = min(tmpl[lane * MT + jj[k]], dlo) + min(tmpl[(lane + 64) * MT + jj[k]], dhi);
                }
#pragma unroll
                for (int off = 32; off >= 1; off >>= 1) {
#pragma unroll
                    for (int k = 0; k < 4; ++k) v[k] += __shfl_xor(v[k], off, 64);
                }
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (lane == k && jj[k] >= 0) ws[d * MT + jj[k]] = v[k];
            }
        }
    }
}

template <int BW, bool ROT, int MODE, bool APPEAR>
__global__ __launch_bounds__(TMAX) void track_kernel(const TrackKernelArgs<APPEAR> a) {
    static_assert(!ROT || BW == 5, "the rotated IoU needs the angle column");
#ifndef MYDET_TRACK_APPEAR_OPTIMAL
    static_assert(!APPEAR || MODE != ASSOC_OPTIMAL, "the fused cost is the instance of track_appear_optimal.hip");
#endif
    extern __shared__ __align__(16) unsigned char track_dyn[];     // AssocLds (ASSOC_OPTIMAL only)
    __shared__ float s_z[5][KMAX];                    // the frame's detections: cx, cy, w, h, angle (0 for BW = 4)
    __shared__ float s_g[ROT ? 7 : 5][KMAX];          // pair-test planes: x1, y1, x2, y2, area | the seven fields of rotiou::Box
    __shared__ float s_sc[KMAX];
    __shared__ int64_t s_cl[KMAX];
    __shared__ int s_order[KMAX];                     // rank -> record slot
    __shared__ int s_dmatch[KMAX];                    // rank -> matched track slot, or -1
    __shared__ int s_bpos[KMAX];                      // k-th birth -> rank
    __shared__ unsigned long long s_red[2][NWMAX];
    __shared__ unsigned long long s_bmask[KMAX / 64], s_fmask[NWMAX];

    const int tid = threadIdx.x, nthr = blockDim.x, lane = tid & 63, wave = tid >> 6, nwave = nthr >> 6;
    const int s = blockIdx.x, MT = a.MT;
    const mydet_track_params &P = a.p;

    // state views (include/mydet.h: the layout is public)
    int32_t *st = a.state + (int64_t)s * a.state_words;
    int64_t *g_cls = reinterpret_cast<int64_t *>(st + MYDET_TRACK_STATE_HEADER);
    int64_t *g_id = g_cls + MT;
    float *g_x = reinterpret_cast<float *>(g_id + MT);
    float *g_v = g_x + 5 * MT, *g_pxx = g_v + 5 * MT, *g_pxv = g_pxx + 5 * MT, *g_pvv = g_pxv + 5 * MT;
    float *g_score = g_pvv + 5 * MT;
    int32_t *g_missed = reinterpret_cast<int32_t *>(g_score + MT);

    const bool slot_ok = tid < MT;
    float x[5], v[5], pxx[5], pxv[5], pvv[5], score = 0.0f;
    int missed = 0;
    int64_t cls = 0, id = 0;
#pragma unroll
    for (int i = 0; i < 5; ++i) { x[i] = v[i] = pxx[i] = pxv[i] = pvv[i] = 0.0f; }
    if (slot_ok) {
        cls = g_cls[tid]; id = g_id[tid];
#pragma unroll
        for (int i = 0; i < 5; ++i) {
            x[i] = g_x[i * MT + tid]; v[i] = g_v[i * MT + tid];
            pxx[i] = g_pxx[i * MT + tid]; pxv[i] = g_pxv[i * MT + tid]; pvv[i] = g_pvv[i * MT + tid];
        }
        score = g_score[tid]; missed = g_missed[tid];
    }
    int64_t next_id = *reinterpret_cast<const int64_t *>(st);
    int nlive = st[2];
    // the appearance state: `has` lives in a register, the template column stays in memory (only this thread touches it)
    [[maybe_unused]] int has = 0;
    [[maybe_unused]] int32_t *tm = nullptr;
    if constexpr (APPEAR) {
        int32_t *as = a.astate + (int64_t)s * a.astate_words;
        tm = as + MT + tid;
        if (slot_ok) has = as[tid];
    }
    // the fused cost: the stream's workspace and its whole template, which the similarity phase reads across the slots
    [[maybe_unused]] int32_t *ws = nullptr;
    [[maybe_unused]] const int32_t *tmpl = nullptr;
    if constexpr (APPEAR && MODE == ASSOC_OPTIMAL) {
        ws = a.sim_ws + (int64_t)s * KMAX * MT;
        tmpl = a.astate + (int64_t)s * a.astate_words + MT;
    }
    const float one_minus_m = 1.0f - P.momentum;

    for (int f = 0; f < a.F; ++f) {
        const int32_t *r = a.rec + (int64_t)s * a.stream_st + (int64_t)f * a.frame_st;
        const int64_t o = (int64_t)s * a.F + f;
        const int cnt = r[MYDET_REC_COUNT];
        if (cnt < 0) {                                             // a bad-class frame: the state stands, the outputs say so
            if (slot_ok) {
                float *ob = a.obox + (o * MT + tid) * 5;
                ob[0] = 0.0f; ob[1] = 0.0f; ob[2] = 0.0f; ob[3] = 0.0f; ob[4] = 0.0f;
                a.oscore[o * MT + tid] = 0.0f; a.ocls[o * MT + tid] = 0; a.oid[o * MT + tid] = 0; a.omissed[o * MT + tid] = -1;
            }
            if constexpr (APPEAR)
                if (slot_ok) { a.osim[o * MT + tid] = -1; a.ohow[o * MT + tid] = -1; }
            if (tid == 0) { a.ocount[o] = MYDET_COUNT_BAD_CLASS; a.odropped[o] = 0; }
            continue;
        }
        const int n = cnt < KMAX ? cnt : KMAX;
        const int n64 = (n + 63) & ~63;
        __syncthreads();                                           // the previous frame is done with the LDS

        // 1. the detections
        for (int d = tid; d < n; d += nthr) {
            const f32x4 b = *reinterpret_cast<const f32x4 *>(r + MYDET_REC_BBOX + 4 * d);
            float ang = 0.0f;
            if constexpr (BW == 5) ang = reinterpret_cast<const float *>(r + MYDET_REC_ANGLE)[d];
            s_z[0][d] = b[0]; s_z[1][d] = b[1]; s_z[2][d] = b[2]; s_z[3][d] = b[3]; s_z[4][d] = ang;
            s_sc[d] = reinterpret_cast<const float *>(r + MYDET_REC_SCORE)[d];
            s_cl[d] = reinterpret_cast<const int64_t *>(r + MYDET_REC_CLASS)[d];
            if constexpr (ROT) {
                const rotiou::Box q = rotiou::make_box(b[0], b[1], b[2], b[3], ang);
                s_g[0][d] = q.cx; s_g[1][d] = q.cy; s_g[2][d] = q.hx; s_g[3][d] = q.hy; s_g[4][d] = q.vx; s_g[5][d] = q.vy;
                s_g[6][d] = q.area;
            } else {
                const float hw = b[2] / 2.0f, hh = b[3] / 2.0f;
                const float x1 = b[0] - hw, y1 = b[1] - hh, x2 = b[0] + hw, y2 = b[1] + hh;
                s_g[0][d] = x1; s_g[1][d] = y1; s_g[2][d] = x2; s_g[3][d] = y2; s_g[4][d] = (x2 - x1) * (y2 - y1);
            }
        }
        if (tid < KMAX / 64) s_bmask[tid] = 0ull;
        if (tid < NWMAX) s_fmask[tid] = 0ull;
        __syncthreads();
        // rank by (score descending, record slot ascending): a total order on the score's bits, so the ranks are a permutation
        for (int d = tid; d < n; d += nthr) {
            const unsigned kd = sortable(s_sc[d]);
            int rank = 0;
            for (int e = 0; e < n; ++e) {
                const unsigned ke = sortable(s_sc[e]);
                rank += (ke > kd || (ke == kd && e < d)) ? 1 : 0;
            }
            s_order[rank] = d;
        }

        // 2. predict (RotBBoxKalmanFilter.predict, then KFTracklet.predict's angle and score rules)
        bool live = slot_ok && id != 0;
        if (live) {
            const float area = x[2] * x[3];
#pragma unroll
            for (int i = 0; i < 5; ++i) {
                const float qx = i < 4 ? P.q[i] * area : P.q[i], qv = i < 4 ? P.q[5 + i] * area : P.q[5 + i];
                const float t = pxv[i] + pvv[i];
                pxx[i] = ((pxx[i] + pxv[i]) + t) + qx;
                pxv[i] = t;
                pvv[i] = pvv[i] + qv;
                x[i] = x[i] + v[i];
            }
            if (a.shift) {                                         // camera motion: the prediction moves with the image
                const int32_t *sh = a.shift + o * 4;
                if (sh[2] == 1) { x[0] = x[0] + (float)sh[0]; x[1] = x[1] + (float)sh[1]; }
            } else if (a.warp) {                                   // the similarity model (include/mydet.h: mydet_track_frames_warp_f32)
                const int32_t *wr = a.warp + o * 8;
                if (wr[6] == 1) {
                    // one rounded operation per line of the header; identity parts are skipped, so that a pure shift row
                    // gives the bits of the branch above (-0.0 + 0.0 would not)
                    constexpr float Q = 1.0f / 65536.0f;
                    const float fa = (float)wr[0] * Q, fb = (float)wr[1] * Q, ftx = (float)wr[2] * Q, fty = (float)wr[3] * Q;
                    const float ux = x[0] - P.img_w * 0.5f, uy = x[1] - P.img_h * 0.5f;
                    x[0] = x[0] + ftx;
                    x[1] = x[1] + fty;
                    if (wr[0] != 0 || wr[1] != 0) {
                        x[0] = x[0] + (fa * ux - fb * uy);
                        x[1] = x[1] + (fb * ux + fa * uy);
                        const float v0 = v[0], v1 = v[1];
                        v[0] = v0 + (fa * v0 - fb * v1);
                        v[1] = v1 + (fb * v0 + fa * v1);
                    }
                    if (wr[4] != 65536) {
                        const float fs = (float)wr[4] * Q;
                        x[2] = x[2] * fs; x[3] = x[3] * fs; v[2] = v[2] * fs; v[3] = v[3] * fs;
                    }
                    if constexpr (BW == 5)
                        if (wr[5] != 0) x[4] = x[4] + (float)wr[5] * Q;
                }
            }
            x[4] = mod180(x[4]);
            if (missed >= 1) score = P.momentum * score;
            missed += 1;
        }
        // the predicted box's side of the pair test
        float t0 = 0.f, t1 = 0.f, t2 = 0.f, t3 = 0.f, t4 = 0.f, t5 = 0.f, t6 = 0.f;
        if (live) {
            if constexpr (ROT) {
                const rotiou::Box q = rotiou::make_box(x[0], x[1], x[2], x[3], x[4]);
                t0 = q.cx; t1 = q.cy; t2 = q.hx; t3 = q.hy; t4 = q.vx; t5 = q.vy; t6 = q.area;
            } else {
                const float hw = x[2] / 2.0f, hh = x[3] / 2.0f;
                t0 = x[0] - hw; t1 = x[1] - hh; t2 = x[0] + hw; t3 = x[1] + hh; t4 = (t2 - t0) * (t3 - t1);
            }
        }
        const int any_live = __syncthreads_or(live ? 1 : 0);      // also: s_order is complete

        // 3. association
        int md = -1;                                               // the record slot this track took
        [[maybe_unused]] int how = 0, simv = -1;                   // APPEAR: the stage that matched, S of the matched pair
        [[maybe_unused]] const uint16_t *dframe = nullptr;
        if constexpr (APPEAR) dframe = a.desc + o * ((int64_t)KMAX * ABINS);
        if constexpr (MODE == ASSOC_OPTIMAL) {
            // Wavefront 0 solves, the others wait at the barrier below; every branch around a barrier is workgroup-uniform
            // (any_live, a.as.bands), and inside the wavefront the solver orders its LDS traffic with HungWaveSync.  No row
            // is skipped and no column compacted: the solver sees the matrix the rule text defines.
            AssocLds &A = *reinterpret_cast<AssocLds *>(track_dyn);
            for (int p = tid; p < n; p += nthr) s_dmatch[p] = -1;
            if (any_live) {
                A.t[0][tid] = t0; A.t[1][tid] = t1; A.t[2][tid] = t2; A.t[3][tid] = t3; A.t[4][tid] = t4; A.t[5][tid] = t5; A.t[6][tid] = t6;
                A.tcls[tid] = cls; A.tmissed[tid] = live ? missed : -1; A.tmd[tid] = -1;
                if constexpr (APPEAR) {
                    // The phase reads template columns that other lanes and waves wrote in steps 4, 5 and 6 of the frame
                    // before: the barrier at the top of the frame released those global stores at workgroup scope.  What it
                    // stores into ws, wavefront 0 reads in the solve: the barrier below.
                    AssocAppearLds &AA = *reinterpret_cast<AssocAppearLds *>(track_dyn);
                    AA.thas[tid] = has;
                    __syncthreads();
                    appear_sim_phase<ROT>(s_g, s_sc, s_cl, AA, n, MT, a.as, P.match_thres, tmpl, dframe, ws, lane, wave, nwave);
                }
                __syncthreads();
                if (wave == 0) {
                    const HungWaveSync wsync;
                    const bool bands = a.as.bands != 0;
                    const unsigned long long before = (1ull << lane) - 1ull;
                    for (int stage = 0; stage < (bands ? 2 : 1); ++stage) {
                        int nr = 0;                                // the stage's rows, in rank order
                        for (int p0 = 0; p0 < n; p0 += 64) {
                            const int p = p0 + lane;
                            int d = 0;
                            bool in = false;
                            if (p < n) {
                                d = s_order[p];
                                const float sc = s_sc[d];
                                const bool high = sc >= a.as.high_thres;
                                in = !bands ? true : stage == 0 ? high : (!high && sc >= a.as.low_thres && sc < a.as.high_thres);
                            }
                            const unsigned long long bal = __ballot(in);
                            if (in) {
                                const int k = nr + __popcll(bal & before);
                                A.rowd[k] = d; A.rowp[k] = p;
                            }
                            nr += __popcll(bal);
                        }
                        wsync();
                        if (nr > 0) {
                            const AssocCost<ROT> iou_cost = {s_g, s_cl, &A, MT, stage == 1, stage == 1 ? a.as.low_match_thres : P.match_thres};
                            const auto cost = [&] {
                                if constexpr (APPEAR)
                                    return AssocAppearCost<ROT>{iou_cost, reinterpret_cast<AssocAppearLds *>(track_dyn)->thas, ws, a.ap.gate, a.weight};
                                else
                                    return iou_cost;
                            }();
                            hung_solve(A.h, nr, MT + nr, cost, lane, wsync);
                            for (int j = lane; j < MT; j += 64) {  // a row on a real column; the costs first: they read tmd
                                const int i = A.h.p[j];
                                A.h.way[j] = i >= 0 && cost(i, j) != ASSOC_INELIGIBLE ? i : -1;
                            }
                            wsync();
                            for (int j = lane; j < MT; j += 64) {
                                const int i = A.h.way[j];
                                if (i >= 0) { A.tmd[j] = A.rowd[i]; s_dmatch[A.rowp[i]] = j; }
                            }
                            wsync();
                        }
                    }
                }
                __syncthreads();
                md = A.tmd[tid];
                if constexpr (APPEAR)
                    if (md >= 0) how = a.as.bands && !(s_sc[md] >= a.as.high_thres) ? 2 : 1;
            }
        } else if (any_live) {
            for (int p = 0; p < n; ++p) {
                const int d = s_order[p];
                unsigned long long key = 0ull;
                bool offered = live && md < 0 && cls == s_cl[d];
                float thres = P.match_thres;
                if constexpr (MODE == ASSOC_GREEDY_BANDS) {
                    const float sc = s_sc[d];
                    if (!(sc >= a.as.high_thres)) {                // stage 2, or a detection that is ignored
                        offered = offered && missed == 1 && sc >= a.as.low_thres && sc < a.as.high_thres;
                        thres = a.as.low_match_thres;
                    }
                }
                if (offered) {
                    float iou;
                    if constexpr (ROT) {
                        const rotiou::Box bi{s_g[0][d], s_g[1][d], s_g[2][d], s_g[3][d], s_g[4][d], s_g[5][d], s_g[6][d]};
                        const rotiou::Box bj{t0, t1, t2, t3, t4, t5, t6};
                        iou = rotiou::rot_iou(bi, bj);
                    } else {
                        const float xx1 = fmaxf(s_g[0][d], t0), yy1 = fmaxf(s_g[1][d], t1);
                        const float xx2 = fminf(s_g[2][d], t2), yy2 = fminf(s_g[3][d], t3);
                        const float ww = fmaxf(0.0f, xx2 - xx1), hh = fmaxf(0.0f, yy2 - yy1);
                        const float inter = ww * hh;
                        iou = inter / (s_g[4][d] + t4 - inter);
                    }
                    if constexpr (APPEAR) {                        // the gate: S only for a pair that passed the IoU test
                        bool pass = iou > thres;
                        if (pass && a.ap.gate > 0 && has) pass = appear_sim(tm, MT, dframe + (int64_t)d * ABINS) >= a.ap.gate;
                        if (pass)
                            key = ((unsigned long long)__float_as_uint(fmaxf(iou, 0.0f)) << 32) | (unsigned)(0xFFFFFFFFu - (unsigned)tid);
                    } else {
                        if (iou > thres)                           // a NaN (0/0) never matches
                            key = ((unsigned long long)__float_as_uint(fmaxf(iou, 0.0f)) << 32) | (unsigned)(0xFFFFFFFFu - (unsigned)tid);
                    }
                }
                key = wave_max(key);
                if (lane == 0) s_red[p & 1][wave] = key;
                __syncthreads();
                unsigned long long best = 0ull;
                for (int w = 0; w < nwave; ++w) { const unsigned long long k = s_red[p & 1][w]; best = k > best ? k : best; }
                const int win = best ? (int)(0xFFFFFFFFu - (unsigned)best) : -1;
                if (win == tid) md = d;
                if (tid == 0) s_dmatch[p] = win;
                if constexpr (APPEAR) {
                    if (win == tid) {
                        how = 1;
                        if constexpr (MODE == ASSOC_GREEDY_BANDS)
                            if (!(s_sc[d] >= a.as.high_thres)) how = 2;
                    }
                }
            }
        } else {
            for (int p = tid; p < n; p += nthr) s_dmatch[p] = -1;
        }

        // 3b. re-identification: a detection that would be born is offered to the lost tracks of its class within reach, the
        // largest S wins (the lowest slot on a tie).  One barrier per candidate; skipped uniformly without one or without a track.
        if constexpr (APPEAR) {
            if (a.ap.reid > 0) {
                __syncthreads();                                   // s_dmatch is complete
                for (int p0 = 0; p0 < n64; p0 += nthr) {
                    const int p = p0 + tid;
                    bool flag = p < n && s_dmatch[p] < 0 && s_sc[s_order[p]] >= P.new_thres;
                    if constexpr (MODE == ASSOC_OPTIMAL) {         // bands are a launch argument there
                        if (a.as.bands) flag = flag && s_sc[s_order[p]] >= a.as.high_thres;
                    } else if constexpr (MODE != ASSOC_GREEDY) flag = flag && s_sc[s_order[p]] >= a.as.high_thres;
                    const unsigned long long bits = __ballot(flag);
                    if (lane == 0 && p < KMAX) s_bmask[p >> 6] = bits;
                }
                const bool elig = live && md < 0 && has && missed >= 2;
                const int any_elig = __syncthreads_or(elig ? 1 : 0);          // also: s_bmask is complete
                int ncand = 0;
#pragma unroll
                for (int w = 0; w < KMAX / 64; ++w) ncand += __popcll(s_bmask[w]);
                if (any_elig && ncand) {
                    int rc = 0;
                    for (int p = 0; p < n; ++p) {
                        if (!((s_bmask[p >> 6] >> (p & 63)) & 1ull)) continue;
                        const int d = s_order[p];
                        unsigned long long key = 0ull;
                        if (live && md < 0 && has && missed >= 2 && cls == s_cl[d]) {
                            const float zw = s_z[2][d], zh = s_z[3][d];
                            const float m = fmaxf(fmaxf(x[2], x[3]), fmaxf(zw, zh));
                            const float lim = a.ap.reach * m;
                            if (fabsf(s_z[0][d] - x[0]) <= lim && fabsf(s_z[1][d] - x[1]) <= lim) {
                                const int sv = appear_sim(tm, MT, dframe + (int64_t)d * ABINS);
                                if (sv >= a.ap.reid) key = ((unsigned long long)(unsigned)sv << 32) | (unsigned)(0xFFFFFFFFu - (unsigned)tid);
                            }
                        }
                        key = wave_max(key);
                        if (lane == 0) s_red[rc & 1][wave] = key;
                        __syncthreads();
                        unsigned long long best = 0ull;
                        for (int w = 0; w < nwave; ++w) { const unsigned long long k = s_red[rc & 1][w]; best = k > best ? k : best; }
                        const int win = best ? (int)(0xFFFFFFFFu - (unsigned)best) : -1;
                        if (win == tid) { md = d; how = 3; }
                        if (tid == 0) s_dmatch[p] = win;
                        ++rc;
                    }
                }
            }
            // S of the matched pair, before the template moves (0 for a track without an appearance: its template is zero)
            if constexpr (MODE == ASSOC_OPTIMAL) {                 // a pair the solve matched was needed: the phase has its S
                if (md >= 0) simv = how == 3 ? appear_sim(tm, MT, dframe + (int64_t)md * ABINS) : has ? ws[md * MT + tid] : 0;
            } else {
                if (md >= 0) simv = appear_sim(tm, MT, dframe + (int64_t)md * ABINS);
            }
        }

        // 4. update the matched tracks (KFTracklet.update)
        if (md >= 0) {
            float z[5];
#pragma unroll
            for (int i = 0; i < 5; ++i) z[i] = s_z[i][md];
            const float za = mod180(z[4]);
            const float c1 = za - 180.0f, c2 = za + 180.0f;
            float zb = za, dmin = fabsf(za - x[4]);
            const float d1 = fabsf(c1 - x[4]), d2 = fabsf(c2 - x[4]);
            if (d1 < dmin) { zb = c1; dmin = d1; }
            if (d2 < dmin) { zb = c2; dmin = d2; }
            z[4] = zb;
            const float area = x[2] * x[3];
#pragma unroll
            for (int i = 0; i < 5; ++i) {
                const float rr = i < 4 ? P.r[i] * area : P.r[i];
                const float y = z[i] - x[i];
                const float inv = 1.0f / (pxx[i] + rr);
                const float kx = pxx[i] * inv, kv = pxv[i] * inv;
                x[i] = x[i] + kx * y;
                v[i] = v[i] + kv * y;
                const float oxx = pxx[i], oxv = pxv[i];
                pxx[i] = oxx - kx * oxx;
                pxv[i] = oxv - kx * oxv;
                pvv[i] = pvv[i] - kv * oxv;
            }
            x[4] = mod180(x[4]);
            if constexpr (APPEAR) {                                // the template follows a detection that could have been born
                if (s_sc[md] >= a.ap.update_thres) {
                    const uint16_t *dr = dframe + (int64_t)md * ABINS;
                    for (int b = 0; b < ABINS; ++b) {
                        const int dv = (int)dr[b] << 8, t = tm[(int64_t)b * MT];
                        tm[(int64_t)b * MT] = has ? t + (((dv - t) * a.ap.alpha) >> 8) : dv;
                    }
                    has = 1;
                }
            }
            score = P.momentum * score + one_minus_m * s_sc[md];
            missed = 0;
        }

        // 5. retire (KFTracklet.is_feasible on the current box, or max_missed frames without a match)
        if (live) {
            const bool bad = score < P.min_score || x[0] < 0.0f || x[1] < 0.0f || x[2] < 0.0f || x[3] < 0.0f || x[0] > P.img_w ||
                             x[1] > P.img_h || x[2] > P.img_w || x[3] > P.img_h || missed >= P.max_missed;
            if (bad) {
                live = false;
#pragma unroll
                for (int i = 0; i < 5; ++i) { x[i] = v[i] = pxx[i] = pxv[i] = pvv[i] = 0.0f; }
                score = 0.0f; missed = 0; cls = 0; id = 0;
                if constexpr (APPEAR) {
                    for (int b = 0; b < ABINS; ++b) tm[(int64_t)b * MT] = 0;
                    has = 0;
                }
            }
        }
        __syncthreads();                                           // s_dmatch is complete

        // 6. births: the k-th unmatched detection above new_thres (in rank order) goes to the k-th lowest free slot
        for (int p0 = 0; p0 < n64; p0 += nthr) {
            const int p = p0 + tid;
            bool flag = p < n && s_dmatch[p] < 0 && s_sc[s_order[p]] >= P.new_thres;
            if constexpr (MODE != ASSOC_GREEDY)                    // with bands only a high detection starts a track
                if (a.as.bands) flag = flag && s_sc[s_order[p]] >= a.as.high_thres;
            const unsigned long long bits = __ballot(flag);
            if (lane == 0 && p < KMAX) s_bmask[p >> 6] = bits;
        }
        {
            const unsigned long long bits = __ballot(slot_ok && !live);
            if (lane == 0) s_fmask[wave] = bits;
        }
        __syncthreads();
        for (int p = tid; p < n; p += nthr)
            if ((s_bmask[p >> 6] >> (p & 63)) & 1ull) s_bpos[prefix_bits(s_bmask, p)] = p;
        __syncthreads();
        int nbirth = 0, nfree = 0;
#pragma unroll
        for (int w = 0; w < KMAX / 64; ++w) nbirth += __popcll(s_bmask[w]);
#pragma unroll
        for (int w = 0; w < NWMAX; ++w) nfree += __popcll(s_fmask[w]);
        const int born = nbirth < nfree ? nbirth : nfree;
        if (slot_ok && !live) {
            const int fr = prefix_bits(s_fmask, tid);
            if (fr < born) {                                       // RotBBoxKalmanFilter.initiate
                const int d = s_order[s_bpos[fr]];
#pragma unroll
                for (int i = 0; i < 5; ++i) x[i] = s_z[i][d];
                x[4] = mod180(x[4]);
                const float area = x[2] * x[3];
#pragma unroll
                for (int i = 0; i < 5; ++i) {
                    v[i] = 0.0f;
                    pxx[i] = i < 4 ? P.p0[i] * area : P.p0[i];
                    pxv[i] = 0.0f;
                    pvv[i] = i < 4 ? P.p0[5 + i] * area : P.p0[5 + i];
                }
                score = s_sc[d]; missed = 0; cls = s_cl[d]; id = next_id + fr;
                live = true;
                if constexpr (APPEAR) {
                    const uint16_t *dr = dframe + (int64_t)d * ABINS;
                    for (int b = 0; b < ABINS; ++b) tm[(int64_t)b * MT] = (int)dr[b] << 8;
                    has = 1; how = 4; simv = -1;
                }
            }
        }
        next_id += born;
        nlive = MT - nfree + born;

        // the frame's outputs
        if (slot_ok) {
            float *ob = a.obox + (o * MT + tid) * 5;
            ob[0] = x[0]; ob[1] = x[1]; ob[2] = x[2]; ob[3] = x[3]; ob[4] = x[4];
            a.oscore[o * MT + tid] = score; a.ocls[o * MT + tid] = cls; a.oid[o * MT + tid] = id;
            a.omissed[o * MT + tid] = live ? missed : -1;
            if constexpr (APPEAR) { a.osim[o * MT + tid] = live ? simv : -1; a.ohow[o * MT + tid] = live ? how : -1; }
        }
        if (tid == 0) { a.ocount[o] = nlive; a.odropped[o] = nbirth - born; }
    }

    if (slot_ok) {
        g_cls[tid] = cls; g_id[tid] = id;
#pragma unroll
        for (int i = 0; i < 5; ++i) {
            g_x[i * MT + tid] = x[i]; g_v[i * MT + tid] = v[i];
            g_pxx[i * MT + tid] = pxx[i]; g_pxv[i * MT + tid] = pxv[i]; g_pvv[i * MT + tid] = pvv[i];
        }
        g_score[tid] = score; g_missed[tid] = missed;
        if constexpr (APPEAR) a.astate[(int64_t)s * a.astate_words + tid] = has;
    }
    if (tid == 0) { *reinterpret_cast<int64_t *>(st) = next_id; st[2] = nlive; }
}

#ifndef MYDET_TRACK_APPEAR
__global__ __launch_bounds__(256) void track_reset_kernel(int32_t *state, int64_t words) {
    int32_t *st = state + (int64_t)blockIdx.x * words;
    for (int64_t i = threadIdx.x; i < words; i += 256) st[i] = i == 0 ? 1 : 0;      // next id 1, everything else 0
}
#endif

}  // namespace

// This file is three translation units (the Makefile builds track_appear.hip, which is this file under MYDET_TRACK_APPEAR, and
// track_appear_optimal.hip, which adds MYDET_TRACK_APPEAR_OPTIMAL): the instances and entry points without an appearance here,
// the greedy ones with it in the second, the optimal assignment on the fused cost in the third.  One unit would do for the language, but
// the compiler's inlining choices inside an instance depend on how many instances share its helpers, and the instances that
// were here before the appearance must stay the code they were (profiles/appearance.md has both builds side by side).
#ifndef MYDET_TRACK_APPEAR
extern "C" int64_t mydet_track_state_words(int max_tracks) {
    if (max_tracks < 1 || max_tracks > MYDET_TRACK_MAX_TRACKS) return 0;
    return ((int64_t)MYDET_TRACK_STATE_HEADER + (int64_t)MYDET_TRACK_SLOT_WORDS * max_tracks + 3) / 4 * 4;
}

extern "C" int mydet_track_reset(int32_t *state, int S, int max_tracks, void *stream) {
    if (S <= 0 || max_tracks < 1 || !state || ((uintptr_t)state & 15)) return MYDET_E_BADARG;
    if (max_tracks > MYDET_TRACK_MAX_TRACKS) return MYDET_E_UNSUPP;
    hipLaunchKernelGGL(track_reset_kernel, dim3((unsigned)S), dim3(256), 0, (hipStream_t)stream, state, mydet_track_state_words(max_tracks));
    return mydet_launch_status();
}
#endif

namespace {

inline bool track_finite(float v) { return v - v == 0.0f; }            // false for a NaN and for an infinity

// One instance: the > 64 KiB LDS opt-in of the optimal assignment is per kernel and per device (common.h)
template <int BW, bool ROT, int MODE, bool APPEAR>
int track_launch(const TrackKernelArgs<APPEAR> &a, dim3 grid, dim3 block, hipStream_t stream) {
    size_t dyn = 0;
    if constexpr (MODE == ASSOC_OPTIMAL) {
        static unsigned long long opted = 0ull;                    // one bit per device ordinal
        dyn = APPEAR ? sizeof(AssocAppearLds) : sizeof(AssocLds);
        const int st = mydet_lds_opt_in(opted, track_kernel<BW, ROT, MODE, APPEAR>, (int)dyn + ASSOC_STATIC_LDS);
        if (st) return st;
    }
    hipLaunchKernelGGL((track_kernel<BW, ROT, MODE, APPEAR>), grid, block, dyn, stream, a);
    return mydet_launch_status();
}

template <int MODE, bool APPEAR = false>
int track_launch_mode(const TrackKernelArgs<APPEAR> &a, int box_width, dim3 grid, dim3 block, hipStream_t stream) {
    if (box_width == 4) return track_launch<4, false, MODE, APPEAR>(a, grid, block, stream);
    if (a.p.match == MYDET_TRACK_MATCH_ROTATED) return track_launch<5, true, MODE, APPEAR>(a, grid, block, stream);
    return track_launch<5, false, MODE, APPEAR>(a, grid, block, stream);
}

// The argument rules every tracker entry point shares; fills `a`
int track_setup(TrackArgs &a, const int32_t *records, int64_t stream_stride_words, int64_t frame_stride_words, int S, int F, int box_width,
                const mydet_track_params *params, int max_tracks, int32_t *state, float *out_box, float *out_score, int64_t *out_class,
                int64_t *out_id, int32_t *out_missed, int32_t *out_count, int32_t *out_dropped, const mydet_track_assoc *assoc,
                const int32_t *shift, const int32_t *warp = nullptr) {
    if (S <= 0 || F <= 0 || max_tracks < 1) return MYDET_E_BADARG;
    if (box_width != 4 && box_width != 5) return MYDET_E_BADARG;
    if (!records || !params || !state || !out_box || !out_score || !out_class || !out_id || !out_missed || !out_count || !out_dropped)
        return MYDET_E_BADARG;
    if (params->match != MYDET_TRACK_MATCH_IOU && params->match != MYDET_TRACK_MATCH_ROTATED) return MYDET_E_BADARG;
    if (params->match == MYDET_TRACK_MATCH_ROTATED && box_width != 5) return MYDET_E_BADARG;
    if (!assoc) return MYDET_E_BADARG;
    if (assoc->assign != MYDET_TRACK_ASSIGN_GREEDY && assoc->assign != MYDET_TRACK_ASSIGN_OPTIMAL) return MYDET_E_BADARG;
    if (assoc->bands != 0 && assoc->bands != 1) return MYDET_E_BADARG;
    if (assoc->bands) {
        if (!track_finite(assoc->high_thres) || !track_finite(assoc->low_thres) || !track_finite(assoc->low_match_thres)) return MYDET_E_BADARG;
        if (assoc->low_thres >= assoc->high_thres) return MYDET_E_BADARG;
    }
    // a record's box plane is read with 16-byte loads: the base and both strides keep that alignment
    if (((uintptr_t)records & 15) || ((uintptr_t)state & 15)) return MYDET_E_BADARG;
    if (stream_stride_words < 0 || frame_stride_words < 0 || (stream_stride_words & 3) || (frame_stride_words & 3)) return MYDET_E_BADARG;
    if (((uintptr_t)out_box & 3) || ((uintptr_t)out_score & 3) || ((uintptr_t)out_class & 7) || ((uintptr_t)out_id & 7) ||
        ((uintptr_t)out_missed & 3) || ((uintptr_t)out_count & 3) || ((uintptr_t)out_dropped & 3) || ((uintptr_t)shift & 3) || ((uintptr_t)warp & 3))
        return MYDET_E_BADARG;
    if (max_tracks > MYDET_TRACK_MAX_TRACKS) return MYDET_E_UNSUPP;
    a.rec = records; a.stream_st = stream_stride_words; a.frame_st = frame_stride_words; a.F = F; a.MT = max_tracks;
    a.p = *params;
    a.state = state; a.state_words = mydet_track_state_words(max_tracks);
    a.obox = out_box; a.oscore = out_score; a.ocls = out_class; a.oid = out_id; a.omissed = out_missed; a.ocount = out_count;
    a.odropped = out_dropped;
    a.as = *assoc;
    a.shift = shift;
    a.warp = warp;
    return 0;
}

}  // namespace

#ifndef MYDET_TRACK_APPEAR
// The entry points with a camera motion: at most one of shift and warp is not null
static int track_frames_camera(const int32_t *records, int64_t stream_stride_words, int64_t frame_stride_words, int S, int F, int box_width,
                               const mydet_track_params *params, int max_tracks, int32_t *state, float *out_box, float *out_score,
                               int64_t *out_class, int64_t *out_id, int32_t *out_missed, int32_t *out_count, int32_t *out_dropped,
                               const mydet_track_assoc *assoc, const int32_t *shift, const int32_t *warp, void *stream) {
    TrackArgs a;
    const int code = track_setup(a, records, stream_stride_words, frame_stride_words, S, F, box_width, params, max_tracks, state, out_box,
                                 out_score, out_class, out_id, out_missed, out_count, out_dropped, assoc, shift, warp);
    if (code) return code;
    const dim3 grid((unsigned)S), block((unsigned)((max_tracks + 63) / 64 * 64));
    if (assoc->assign == MYDET_TRACK_ASSIGN_OPTIMAL) return track_launch_mode<ASSOC_OPTIMAL>(a, box_width, grid, block, (hipStream_t)stream);
    if (assoc->bands) return track_launch_mode<ASSOC_GREEDY_BANDS>(a, box_width, grid, block, (hipStream_t)stream);
    return track_launch_mode<ASSOC_GREEDY>(a, box_width, grid, block, (hipStream_t)stream);
}

extern "C" int mydet_track_frames_motion_f32(const int32_t *records, int64_t stream_stride_words, int64_t frame_stride_words, int S, int F,
                                             int box_width, const mydet_track_params *params, int max_tracks, int32_t *state,
                                             float *out_box, float *out_score, int64_t *out_class, int64_t *out_id, int32_t *out_missed,
                                             int32_t *out_count, int32_t *out_dropped, const mydet_track_assoc *assoc, const int32_t *shift,
                                             void *stream) {
    return track_frames_camera(records, stream_stride_words, frame_stride_words, S, F, box_width, params, max_tracks, state, out_box, out_score,
                               out_class, out_id, out_missed, out_count, out_dropped, assoc, shift, nullptr, stream);
}

extern "C" int mydet_track_frames_warp_f32(const int32_t *records, int64_t stream_stride_words, int64_t frame_stride_words, int S, int F,
                                           int box_width, const mydet_track_params *params, int max_tracks, int32_t *state,
                                           float *out_box, float *out_score, int64_t *out_class, int64_t *out_id, int32_t *out_missed,
                                           int32_t *out_count, int32_t *out_dropped, const mydet_track_assoc *assoc, const int32_t *warp,
                                           void *stream) {
    return track_frames_camera(records, stream_stride_words, frame_stride_words, S, F, box_width, params, max_tracks, state, out_box, out_score,
                               out_class, out_id, out_missed, out_count, out_dropped, assoc, nullptr, warp, stream);
}

#else
#ifndef MYDET_TRACK_APPEAR_OPTIMAL
extern "C" int64_t mydet_track_appear_state_words(int max_tracks) {
    if (max_tracks < 1 || max_tracks > MYDET_TRACK_MAX_TRACKS) return 0;
    return ((int64_t)(1 + MYDET_APPEAR_BINS) * max_tracks + 3) / 4 * 4;
}
#endif

namespace {

// The argument rules of the appearance that both of its entry points share, behind track_setup's; fills the rest of `a`
int track_appear_setup(TrackAppearArgs &a, int max_tracks, const mydet_track_appear *appear, const uint16_t *desc, int32_t *appear_state,
                       int32_t *out_sim, int32_t *out_how) {
    if (!appear || !desc || !appear_state || !out_sim || !out_how) return MYDET_E_BADARG;
    if (((uintptr_t)desc & 15) || ((uintptr_t)appear_state & 15) || ((uintptr_t)out_sim & 3) || ((uintptr_t)out_how & 3)) return MYDET_E_BADARG;
    if (appear->gate < 0 || appear->gate > MYDET_APPEAR_SIM_MAX || appear->reid < 0 || appear->reid > MYDET_APPEAR_SIM_MAX) return MYDET_E_BADARG;
    if (appear->alpha < 1 || appear->alpha > 256) return MYDET_E_BADARG;
    if (!track_finite(appear->reach) || appear->reach < 0.0f || appear->update_thres != appear->update_thres) return MYDET_E_BADARG;
    a.ap = *appear; a.desc = desc; a.astate = appear_state; a.astate_words = mydet_track_appear_state_words(max_tracks);
    a.osim = out_sim; a.ohow = out_how;
    return 0;
}

}  // namespace

#ifndef MYDET_TRACK_APPEAR_OPTIMAL
static int track_frames_appear_camera(const int32_t *records, int64_t stream_stride_words, int64_t frame_stride_words, int S, int F,
                                      int box_width, const mydet_track_params *params, int max_tracks, int32_t *state, float *out_box,
                                      float *out_score, int64_t *out_class, int64_t *out_id, int32_t *out_missed, int32_t *out_count,
                                      int32_t *out_dropped, const mydet_track_assoc *assoc, const int32_t *shift, const int32_t *warp,
                                      const mydet_track_appear *appear, const uint16_t *desc, int32_t *appear_state, int32_t *out_sim,
                                      int32_t *out_how, void *stream) {
    TrackAppearArgs a;
    const int code = track_setup(a, records, stream_stride_words, frame_stride_words, S, F, box_width, params, max_tracks, state, out_box,
                                 out_score, out_class, out_id, out_missed, out_count, out_dropped, assoc, shift, warp);
    if (code) return code;
    const int acode = track_appear_setup(a, max_tracks, appear, desc, appear_state, out_sim, out_how);
    if (acode) return acode;
    if (assoc->assign != MYDET_TRACK_ASSIGN_GREEDY) return MYDET_E_UNSUPP;          // mydet_track_frames_appear_optimal_f32 has the fused cost
    const dim3 grid((unsigned)S), block((unsigned)((max_tracks + 63) / 64 * 64));
    if (assoc->bands) return track_launch_mode<ASSOC_GREEDY_BANDS, true>(a, box_width, grid, block, (hipStream_t)stream);
    return track_launch_mode<ASSOC_GREEDY, true>(a, box_width, grid, block, (hipStream_t)stream);
}

extern "C" int mydet_track_frames_appear_f32(const int32_t *records, int64_t stream_stride_words, int64_t frame_stride_words, int S, int F,
                                             int box_width, const mydet_track_params *params, int max_tracks, int32_t *state,
                                             float *out_box, float *out_score, int64_t *out_class, int64_t *out_id, int32_t *out_missed,
                                             int32_t *out_count, int32_t *out_dropped, const mydet_track_assoc *assoc, const int32_t *shift,
                                             const mydet_track_appear *appear, const uint16_t *desc, int32_t *appear_state,
                                             int32_t *out_sim, int32_t *out_how, void *stream) {
    return track_frames_appear_camera(records, stream_stride_words, frame_stride_words, S, F, box_width, params, max_tracks, state, out_box,
                                      out_score, out_class, out_id, out_missed, out_count, out_dropped, assoc, shift, nullptr, appear, desc,
                                      appear_state, out_sim, out_how, stream);
}

extern "C" int mydet_track_frames_appear_warp_f32(const int32_t *records, int64_t stream_stride_words, int64_t frame_stride_words, int S,
                                                  int F, int box_width, const mydet_track_params *params, int max_tracks, int32_t *state,
                                                  float *out_box, float *out_score, int64_t *out_class, int64_t *out_id,
                                                  int32_t *out_missed, int32_t *out_count, int32_t *out_dropped,
                                                  const mydet_track_assoc *assoc, const int32_t *warp, const mydet_track_appear *appear,
                                                  const uint16_t *desc, int32_t *appear_state, int32_t *out_sim, int32_t *out_how,
                                                  void *stream) {
    return track_frames_appear_camera(records, stream_stride_words, frame_stride_words, S, F, box_width, params, max_tracks, state, out_box,
                                      out_score, out_class, out_id, out_missed, out_count, out_dropped, assoc, nullptr, warp, appear, desc,
                                      appear_state, out_sim, out_how, stream);
}
#else
extern "C" int64_t mydet_track_appear_ws_words(int max_tracks) {
    if (max_tracks < 1 || max_tracks > MYDET_TRACK_MAX_TRACKS) return 0;
    return (int64_t)MYDET_REC_TOPK * max_tracks;
}

static int track_frames_appear_optimal_camera(const int32_t *records, int64_t stream_stride_words, int64_t frame_stride_words, int S, int F,
                                              int box_width, const mydet_track_params *params, int max_tracks, int32_t *state,
                                              float *out_box, float *out_score, int64_t *out_class, int64_t *out_id, int32_t *out_missed,
                                              int32_t *out_count, int32_t *out_dropped, const mydet_track_assoc *assoc, const int32_t *shift,
                                              const int32_t *warp, const mydet_track_appear *appear, const uint16_t *desc,
                                              int32_t *appear_state, int32_t *out_sim, int32_t *out_how, int weight, int32_t *sim_ws,
                                              void *stream) {
    TrackAppearArgs a;
    const int code = track_setup(a, records, stream_stride_words, frame_stride_words, S, F, box_width, params, max_tracks, state, out_box,
                                 out_score, out_class, out_id, out_missed, out_count, out_dropped, assoc, shift, warp);
    if (code) return code;
    const int acode = track_appear_setup(a, max_tracks, appear, desc, appear_state, out_sim, out_how);
    if (acode) return acode;
    if (weight < 0 || weight > 256 || !sim_ws || ((uintptr_t)sim_ws & 15)) return MYDET_E_BADARG;
    if (assoc->assign != MYDET_TRACK_ASSIGN_OPTIMAL) return MYDET_E_UNSUPP;         // the walk's key stays IoU-major
    a.weight = weight; a.sim_ws = sim_ws;
    const dim3 grid((unsigned)S), block((unsigned)((max_tracks + 63) / 64 * 64));
    return track_launch_mode<ASSOC_OPTIMAL, true>(a, box_width, grid, block, (hipStream_t)stream);
}

extern "C" int mydet_track_frames_appear_optimal_f32(const int32_t *records, int64_t stream_stride_words, int64_t frame_stride_words, int S,
                                                     int F, int box_width, const mydet_track_params *params, int max_tracks, int32_t *state,
                                                     float *out_box, float *out_score, int64_t *out_class, int64_t *out_id,
                                                     int32_t *out_missed, int32_t *out_count, int32_t *out_dropped,
                                                     const mydet_track_assoc *assoc, const int32_t *shift, const mydet_track_appear *appear,
                                                     const uint16_t *desc, int32_t *appear_state, int32_t *out_sim, int32_t *out_how,
                                                     int weight, int32_t *sim_ws, void *stream) {
    return track_frames_appear_optimal_camera(records, stream_stride_words, frame_stride_words, S, F, box_width, params, max_tracks, state,
                                              out_box, out_score, out_class, out_id, out_missed, out_count, out_dropped, assoc, shift, nullptr,
                                              appear, desc, appear_state, out_sim, out_how, weight, sim_ws, stream);
}

extern "C" int mydet_track_frames_appear_optimal_warp_f32(const int32_t *records, int64_t stream_stride_words, int64_t frame_stride_words,
                                                          int S, int F, int box_width, const mydet_track_params *params, int max_tracks,
                                                          int32_t *state, float *out_box, float *out_score, int64_t *out_class,
                                                          int64_t *out_id, int32_t *out_missed, int32_t *out_count, int32_t *out_dropped,
                                                          const mydet_track_assoc *assoc, const int32_t *warp,
                                                          const mydet_track_appear *appear, const uint16_t *desc, int32_t *appear_state,
                                                          int32_t *out_sim, int32_t *out_how, int weight, int32_t *sim_ws, void *stream) {
    return track_frames_appear_optimal_camera(records, stream_stride_words, frame_stride_words, S, F, box_width, params, max_tracks, state,
                                              out_box, out_score, out_class, out_id, out_missed, out_count, out_dropped, assoc, nullptr, warp,
                                              appear, desc, appear_state, out_sim, out_how, weight, sim_ws, stream);
}
#endif

#endif

#ifndef MYDET_TRACK_APPEAR
extern "C" int mydet_track_frames_assoc_f32(const int32_t *records, int64_t stream_stride_words, int64_t frame_stride_words, int S, int F,
                                            int box_width, const mydet_track_params *params, int max_tracks, int32_t *state,
                                            float *out_box, float *out_score, int64_t *out_class, int64_t *out_id, int32_t *out_missed,
                                            int32_t *out_count, int32_t *out_dropped, const mydet_track_assoc *assoc, void *stream) {
    return mydet_track_frames_motion_f32(records, stream_stride_words, frame_stride_words, S, F, box_width, params, max_tracks, state, out_box,
                                         out_score, out_class, out_id, out_missed, out_count, out_dropped, assoc, nullptr, stream);
}

extern "C" int mydet_track_frames_f32(const int32_t *records, int64_t stream_stride_words, int64_t frame_stride_words, int S, int F,
                                      int box_width, const mydet_track_params *params, int max_tracks, int32_t *state,
                                      float *out_box, float *out_score, int64_t *out_class, int64_t *out_id, int32_t *out_missed,
                                      int32_t *out_count, int32_t *out_dropped, void *stream) {
    const mydet_track_assoc assoc = {MYDET_TRACK_ASSIGN_GREEDY, 0, 0.0f, 0.0f, 0.0f, {0, 0, 0}};
    return mydet_track_frames_assoc_f32(records, stream_stride_words, frame_stride_words, S, F, box_width, params, max_tracks, state, out_box,
                                        out_score, out_class, out_id, out_missed, out_count, out_dropped, &assoc, stream);
}
#endif
