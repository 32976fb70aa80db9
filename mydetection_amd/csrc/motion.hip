// Global camera motion from the frames themselves: one integer shift (dx, dy) per frame, for the tracker's predict step
// (include/mydet.h: mydet_motion_frames_rgb_u8 has the rules, DESIGN.md section 4 the reasoning; tests/_motion_ref.py restates
// them in Python integers and every output and the state equal it with ==).
//
// All S*F frames of a call are parallel work: a frame depends only on the luma of its predecessor, which is another frame of
// the call or, for f = 0, the stream's state.  Five launches, because the rules have two frame-wide medians in the middle:
//   1. motion_reduce_kernel   every frame -> its reduced luma (k x k box means) in the workspace.  The one pass over whole frames:
//                             a thread makes four neighbouring reduced pixels (one dword store) from k rows of 4k pixels, read
//                             with 8- or 16-byte loads when the frames allow it; every frame byte is read once.
//   2. motion_coarse_kernel   one workgroup per block: the 16 x 16 block of the previous reduced luma and the (16 + 2R)^2 window
//                             of the current one sit in LDS, work items (candidate, quarter of the rows) spread over the lanes,
//                             SADs four bytes at a time (v_sad_u8; the window row is read as aligned dwords and shifted with
//                             v_alignbyte_b32), partial sums meet by LDS atomics, the best key by shuffles.
//   3. motion_median_kernel   one workgroup per frame: validity of every block, then the lower median of (cdx, cdy) by a
//                             histogram -- the values live in [-R, R], so counting replaces sorting.
//   4. motion_refine_kernel   one workgroup per valid block: the P x P patch of the previous luma and the (P + 2k)^2 window of
//                             the current luma at D k, at full resolution, through the same SAD core.
//   5. motion_finish_kernel   per frame the median of the block vectors -> out_shift; further workgroups write the state of
//                             the stream's last frame (reduced luma and the patches).  The state is written only here, after
//                             every reader of the old state has run (stream order), so no frame of the call sees a torn state.
// Launches 3 and 5 are tiny; merging them into their producers would need a grid-wide "last workgroup" protocol for a few
// microseconds (profiles/motion.md has the numbers).
//
// The similarity model (mydet_motion_warp_frames_*; tests/_warp_ref.py restates it) keeps launches 1 - 3, refines every block
// around its OWN coarse vector (under rotation the block vectors differ by far more than k), and puts motion_fit_kernel, one
// workgroup per frame, between the refine and the finish launch, which then only writes the state: medians by counting ranks
// (the Q16 values have no small range for a histogram), two rounds of closed-form least squares on the block lattice, the zoom
// and the angle from an integer square root and an integer arctangent polynomial.  profiles/motion_warp.md has the numbers.
#include "common.h"
#include "yuv_fetch.h"

namespace {

constexpr int NB_MAX = MYDET_MOTION_MAX_BLOCKS;
constexpr int R_MAX = MYDET_MOTION_MAX_SEARCH;
constexpr int CAND_MAX = (2 * R_MAX + 1) * (2 * R_MAX + 1);          // 1089 coarse candidates; the refine stage has at most 289
constexpr int NPART = 4;                                             // a candidate's rows are summed in four parts
constexpr int BINS_MAX = 2 * (R_MAX * 8 + 8) + 1;                    // block vectors live in [-(R k + k), R k + k]
constexpr int SAVE_GROUPS = 32;                                      // workgroups per stream that write the state
constexpr int ST_HEADER = MYDET_MOTION_STATE_HEADER;
constexpr int64_t MOTION_T_LIMIT = 1 << 24;                          // Q16: a fitted translation of 256 pixels or more is no result

// Geometry of the rules for one frame size (include/mydet.h)
struct Geo {
    int H, W, k, lk2, R, hr, wr, wrp, nby, nbx, nb, P;
    int64_t red_bytes, patch_bytes;                                  // per frame: hr * wrp; nb * P * P
};

int motion_geo(Geo &g, int H, int W, int k, int R) {
    if (H < 1 || W < 1 || H > MYDET_ZONE_MAX_FRAME || W > MYDET_ZONE_MAX_FRAME) return MYDET_E_BADARG;
    if (k != 2 && k != 4 && k != 8) return MYDET_E_BADARG;
    if (R < MYDET_MOTION_MIN_SEARCH || R > MYDET_MOTION_MAX_SEARCH) return MYDET_E_BADARG;
    g.H = H; g.W = W; g.k = k; g.lk2 = k == 2 ? 2 : k == 4 ? 4 : 6; g.R = R;
    g.hr = H / k; g.wr = W / k; g.wrp = (g.wr + 3) & ~3;
    if (g.hr < 2 * R + 16 || g.wr < 2 * R + 16) return MYDET_E_BADARG;
    g.nby = (g.hr - 2 * R) / 16; g.nbx = (g.wr - 2 * R) / 16; g.nb = g.nby * g.nbx;
    if (g.nb > NB_MAX) return MYDET_E_UNSUPP;
    g.P = 8 * k < 32 ? 8 * k : 32;
    g.red_bytes = (int64_t)g.hr * g.wrp;
    g.patch_bytes = (int64_t)g.nb * g.P * g.P;
    return 0;
}

int motion_default_reduce(int H, int W) {
    const int m = H > W ? H : W;
    return m <= 1024 ? 2 : m <= 2048 ? 4 : 8;
}

int64_t motion_state_words(const Geo &g) { return ((int64_t)ST_HEADER + g.red_bytes / 4 + g.patch_bytes / 4 + 3) / 4 * 4; }

// workspace: reduced lumas [frames][hr * wrp] bytes | frame info int32 [frames][4] (Dx, Dy, ok, n_valid) | blocks int32 [frames][nb][6]
struct Ws { int64_t red, info, blocks, total; };
Ws motion_ws(const Geo &g, int64_t frames) {
    Ws w;
    w.red = 0;
    w.info = (frames * g.red_bytes + 15) / 16 * 16;
    w.blocks = w.info + frames * 16;
    w.total = w.blocks + frames * g.nb * 24;
    return w;
}

// ---- the luma of a pixel, per source ----

struct RgbLuma {
    const unsigned char *p;
    int64_t img, row;
    int wide;                                                        // base, pitch and frame stride allow the 8- / 16-byte loads
    __device__ __forceinline__ uint32_t at(int o, int y, int x) const {
        const unsigned char *q = p + (int64_t)o * img + (int64_t)y * row + 3 * (int64_t)x;
        return (77u * q[0] + 150u * q[1] + 29u * q[2] + 128u) >> 8;
    }
};

template <int BPS, bool PLANAR>
struct YuvLuma {
    YuvSrc s;
    __device__ __forceinline__ uint32_t at(int o, int y, int x) const {
        return yuv_samples<BPS, PLANAR, 2>(s.p[0] + (int64_t)o * s.img[0] + (int64_t)y * s.row[0] + (int64_t)x * BPS, 1, 0);
    }
};

__device__ __forceinline__ uint32_t byte_of(const uint32_t *w, int b) { return (w[b >> 2] >> (8 * (b & 3))) & 255u; }

// acc[j] += the K lumas of reduced pixel j (j < n) in source row y, from source column x0 on
template <int K>
__device__ __forceinline__ void row_sums(const RgbLuma &s, int o, int y, int x0, int n, uint32_t acc[4]) {
    const unsigned char *q = s.p + (int64_t)o * s.img + (int64_t)y * s.row + 3 * (int64_t)x0;
    if (s.wide && n == 4) {
        uint32_t w[3 * K];                                           // 4K pixels = 12K bytes
        if constexpr (K == 2) {
#pragma unroll
            for (int i = 0; i < 3; ++i) { const uint2 t = reinterpret_cast<const uint2 *>(q)[i]; w[2 * i] = t.x; w[2 * i + 1] = t.y; }
        } else {
#pragma unroll
            for (int i = 0; i < 3 * K / 4; ++i) {
                const uint4 t = reinterpret_cast<const uint4 *>(q)[i];
                w[4 * i] = t.x; w[4 * i + 1] = t.y; w[4 * i + 2] = t.z; w[4 * i + 3] = t.w;
            }
        }
#pragma unroll
        for (int px = 0; px < 4 * K; ++px)
            acc[px / K] += (77u * byte_of(w, 3 * px) + 150u * byte_of(w, 3 * px + 1) + 29u * byte_of(w, 3 * px + 2) + 128u) >> 8;
    } else {
        for (int j = 0; j < n; ++j)
            for (int i = 0; i < K; ++i) {
                const unsigned char *c = q + 3 * (j * K + i);
                acc[j] += (77u * c[0] + 150u * c[1] + 29u * c[2] + 128u) >> 8;
            }
    }
}

template <int K, int BPS, bool PLANAR>
__device__ __forceinline__ void row_sums(const YuvLuma<BPS, PLANAR> &s, int o, int y, int x0, int n, uint32_t acc[4]) {
    const unsigned char *q = s.s.p[0] + (int64_t)o * s.s.img[0] + (int64_t)y * s.s.row[0] + (int64_t)x0 * BPS;
    const int valid = n * K;                                         // samples from x0 on that the rules read
#pragma unroll
    for (int d = 0; d < K; ++d) {                                    // 4K samples, four at a time as packed bytes
        if (4 * d >= valid) break;
        const uint32_t w = yuv_samples<BPS, PLANAR, 4>(q + 4 * d * BPS, valid - 4 * d, s.s.wide);
        if constexpr (K == 2) {
            acc[2 * d] = __builtin_amdgcn_sad_u8(w & 0xffffu, 0u, acc[2 * d]);
            acc[2 * d + 1] = __builtin_amdgcn_sad_u8(w >> 16, 0u, acc[2 * d + 1]);
        } else {
            acc[d / (K / 4)] = __builtin_amdgcn_sad_u8(w, 0u, acc[d / (K / 4)]);
        }
    }
}

struct MotionArgs {
    Geo g;
    int S, F;
    int min_texture, min_blocks;
    int32_t *state;
    int64_t state_words;
    unsigned char *red;                                              // workspace
    int32_t *info, *blocks;                                          // blocks: out_blocks, or the workspace's
    int32_t *oshift;
    int model;                                                       // 0: the shift; 1: the similarity, with the fields below
    int tol_q, zoom_q, rot_q;                                        // Q16: pixels, |s - 1|, degrees
    int32_t *owarp, *oinl;                                           // oinl may be null
};

// 1. reduced luma: thread = four neighbouring reduced pixels of one row
template <int K, typename Src>
__global__ __launch_bounds__(256) void motion_reduce_kernel(const Src src, const MotionArgs a) {
    const Geo &g = a.g;
    const int wq = g.wrp >> 2, o = blockIdx.y;
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= g.hr * wq) return;
    const int i = idx / wq, jq = idx - i * wq;
    const int n = g.wr - 4 * jq < 4 ? g.wr - 4 * jq : 4;             // >= 1: wrp - wr < 4
    uint32_t acc[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int r = 0; r < K; ++r) row_sums<K>(src, o, i * K + r, 4 * jq * K, n, acc);
    uint32_t v = 0u;
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (j < n) v |= ((acc[j] + (uint32_t)(K * K / 2)) >> g.lk2) << (8 * j);
    reinterpret_cast<uint32_t *>(a.red + (int64_t)o * g.red_bytes)[idx] = v;      // idx = i * wq + jq
}

// The previous reduced luma of frame o = s*F + f, or null for a stream's first frame after a reset
__device__ __forceinline__ const unsigned char *prev_reduced(const MotionArgs &a, int s, int f) {
    if (f > 0) return a.red + (int64_t)(s * a.F + f - 1) * a.g.red_bytes;
    const int32_t *st = a.state + (int64_t)s * a.state_words;
    return st[0] ? reinterpret_cast<const unsigned char *>(st + ST_HEADER) : nullptr;
}

__device__ __forceinline__ int lds_pitch_dwords(int bytes) { return (((bytes + 3) >> 2) + 1) | 1; }

// SAD of rows [r0, r1) of a template of BW dwords per row (LDS, pitch BW) against the window (LDS, pitch wp dwords) at row
// offset cy and byte offset cx: aligned dword reads, the bytes shifted into place
template <int BW>
__device__ __forceinline__ uint32_t sad_rows(const uint32_t *tpl, const uint32_t *win, int wp, int r0, int r1, int cy, int cx) {
    const int a0 = cx >> 2, sh = cx & 3;
    uint32_t sad = 0u;
    for (int r = r0; r < r1; ++r) {
        const uint32_t *wr = win + (r + cy) * wp + a0, *tr = tpl + r * BW;
        uint32_t lo = wr[0];
#pragma unroll
        for (int i = 0; i < BW; ++i) {
            const uint32_t hi = wr[i + 1];
            sad = __builtin_amdgcn_sad_u8(__builtin_amdgcn_alignbyte(hi, lo, (uint32_t)sh), tr[i], sad);
            lo = hi;
        }
    }
    return sad;
}

__device__ __forceinline__ unsigned long long wave_min_u64(unsigned long long v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const unsigned long long o = __shfl_xor(v, off, 64);
        v = o < v ? o : v;
    }
    return v;
}

__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const uint32_t o = (uint32_t)__shfl_xor((int)v, off, 64);
        v = o > v ? o : v;
    }
    return v;
}

// The search of one stage over (2 r + 1)^2 candidates whose partial SADs are complete in s_sad: the smallest key
// (SAD, dy^2 + dx^2, dy, dx) and the largest SAD, in every thread.  Key: SAD << 24 | dist << 12 | (dy + r) << 6 | (dx + r).
__device__ __forceinline__ void best_candidate(const uint32_t *s_sad, int r, unsigned long long *s_key, uint32_t *s_max,
                                               unsigned long long &best, uint32_t &smax) {
    const int side = 2 * r + 1, ncand = side * side, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    unsigned long long key = ~0ull;
    uint32_t mx = 0u;
    for (int c = tid; c < ncand; c += 256) {
        const int dy = c / side - r, dx = c % side - r;
        const uint32_t sad = s_sad[c];
        const unsigned long long kk = ((unsigned long long)sad << 24) | ((unsigned long long)(dy * dy + dx * dx) << 12) |
                                      ((unsigned long long)(dy + r) << 6) | (unsigned long long)(dx + r);
        key = kk < key ? kk : key;
        mx = sad > mx ? sad : mx;
    }
    key = wave_min_u64(key);
    mx = wave_max_u32(mx);
    if (lane == 0) { s_key[wave] = key; s_max[wave] = mx; }
    __syncthreads();
    best = s_key[0]; smax = s_max[0];
#pragma unroll
    for (int w = 1; w < 4; ++w) { best = s_key[w] < best ? s_key[w] : best; smax = s_max[w] > smax ? s_max[w] : smax; }
}

// 2. coarse stage: one workgroup per (block, frame)
__global__ __launch_bounds__(256) void motion_coarse_kernel(const MotionArgs a) {
    constexpr int WIN_MAX = 16 + 2 * R_MAX;                          // 48 rows of at most 13 dwords
    __shared__ uint32_t s_tpl[16 * 4];
    __shared__ uint32_t s_win[WIN_MAX * 13];
    __shared__ uint32_t s_sad[CAND_MAX];
    __shared__ unsigned long long s_key[4];
    __shared__ uint32_t s_max[4];
    const Geo &g = a.g;
    const int tid = threadIdx.x, b = blockIdx.x, o = blockIdx.y, s = o / a.F, f = o - s * a.F;
    int32_t *ob = a.blocks + ((int64_t)o * g.nb + b) * 6;
    const unsigned char *prev = prev_reduced(a, s, f);               // workgroup-uniform
    if (!prev) {
        if (tid < 6) ob[tid] = 0;
        return;
    }
    const int R = g.R, side = 2 * R + 1, ncand = side * side, wside = 16 + 2 * R, wp = lds_pitch_dwords(wside);
    const int by = b / g.nbx, bx = b - by * g.nbx, y0 = R + 16 * by, x0 = R + 16 * bx;
    const unsigned char *cur = a.red + (int64_t)o * g.red_bytes;
    // the template: bytes (x0 need not be a multiple of 4); the window: its rows begin at column 16 bx, a dword boundary
    reinterpret_cast<unsigned char *>(s_tpl)[tid] = prev[(int64_t)(y0 + (tid >> 4)) * g.wrp + x0 + (tid & 15)];
    const int wd = (wside + 3) >> 2;                                 // dwords read per row: inside the row's pitch wrp
    for (int i = tid; i < wside * wp; i += 256) {
        const int r = i / wp, c = i - r * wp;
        s_win[i] = c < wd ? reinterpret_cast<const uint32_t *>(cur + (int64_t)(y0 - R + r) * g.wrp + 16 * bx)[c] : 0u;
    }
    for (int c = tid; c < ncand; c += 256) s_sad[c] = 0u;
    __syncthreads();
    for (int w = tid; w < ncand * NPART; w += 256) {
        const int c = w / NPART, part = w - c * NPART;
        const int dy = c / side, dx = c - dy * side;                 // offsets from the window's origin: (dy - R) + R
        atomicAdd(&s_sad[c], sad_rows<4>(s_tpl, s_win, wp, 4 * part, 4 * part + 4, dy, dx));
    }
    __syncthreads();
    unsigned long long best;
    uint32_t smax;
    best_candidate(s_sad, R, s_key, s_max, best, smax);
    if (tid == 0) {
        ob[0] = (int)(best & 63u) - R; ob[1] = (int)((best >> 6) & 63u) - R; ob[2] = (int)(best >> 24); ob[3] = (int)smax;
        ob[4] = 0; ob[5] = 0;
    }
}

__device__ __forceinline__ bool block_valid(const int32_t *blk, int min_texture) {
    return blk[3] - blk[2] >= min_texture && 2 * blk[2] <= blk[3];
}

// The component-wise lower median of fields (fx, fx + 1) of a frame's valid blocks, values in [-lim, lim]; returns n_valid in
// every thread, the medians through mx, my (0 with no valid block).  One workgroup of 256 threads.
__device__ __forceinline__ int block_median(const int32_t *blk, int nb, int fx, int lim, int min_texture, int *s_hist, int *s_out,
                                            int &mx, int &my) {
    const int tid = threadIdx.x, nbins = 2 * lim + 1;
    for (int i = tid; i < 2 * BINS_MAX; i += 256) s_hist[i] = 0;
    if (tid < 3) s_out[tid] = 0;
    __syncthreads();
    for (int b = tid; b < nb; b += 256) {
        const int32_t *q = blk + (int64_t)b * 6;
        if (block_valid(q, min_texture)) {
            atomicAdd(&s_hist[q[fx] + lim], 1);
            atomicAdd(&s_hist[BINS_MAX + q[fx + 1] + lim], 1);
            atomicAdd(&s_out[2], 1);
        }
    }
    __syncthreads();
    const int n = s_out[2];
    if (n > 0) {
        const int m = (n - 1) / 2;
        for (int t = tid; t < 2 * nbins; t += 256) {                 // bin t of x, then of y: the one that holds index m
            const int comp = t >= nbins ? 1 : 0, bin = t - comp * nbins;
            const int *h = s_hist + comp * BINS_MAX;
            int below = 0;
            for (int u = 0; u < bin; ++u) below += h[u];
            if (below <= m && m < below + h[bin]) s_out[comp] = bin - lim;
        }
    }
    __syncthreads();
    mx = s_out[0]; my = s_out[1];
    return n;
}

// 3. coarse median: one workgroup per frame -> info = (Dx, Dy, ok, n_valid)
__global__ __launch_bounds__(256) void motion_median_kernel(const MotionArgs a) {
    __shared__ int s_hist[2 * BINS_MAX];
    __shared__ int s_out[3];
    const int o = blockIdx.x, s = o / a.F, f = o - s * a.F;
    int32_t *info = a.info + (int64_t)o * 4;
    if (!prev_reduced(a, s, f)) {
        if (threadIdx.x < 4) info[threadIdx.x] = 0;
        return;
    }
    int dx, dy;
    const int n = block_median(a.blocks + (int64_t)o * a.g.nb * 6, a.g.nb, 0, a.g.R, a.min_texture, s_hist, s_out, dx, dy);
    if (threadIdx.x == 0) {
        const bool ok = n >= a.min_blocks;
        info[0] = ok ? dx : 0; info[1] = ok ? dy : 0; info[2] = ok ? 1 : 0; info[3] = n;
    }
}

// 4. refine stage: one workgroup per (block, frame), valid blocks of frames with a coarse result only
// OWN (the similarity model): the window sits at the block's own coarse vector instead of the frame's median D.  |c| <= R as
// |D| <= R, so the geometry argument is the same: rows py + c.y K - K .. + P + 2K lie in [3K, (hr - 3) K] (P <= 8K, 16 nby <= hr - 2R).
template <int K, typename Src, bool OWN>
__global__ __launch_bounds__(256) void motion_refine_kernel(const Src src, const MotionArgs a) {
    constexpr int P = 8 * K < 32 ? 8 * K : 32, BW = P / 4, WS = P + 2 * K, SIDE = 2 * K + 1, NCAND = SIDE * SIDE;
    constexpr int WP = (((WS + 3) >> 2) + 1) | 1;
    __shared__ uint32_t s_tpl[P * BW];
    __shared__ uint32_t s_win[WS * WP];
    __shared__ uint32_t s_sad[NCAND];
    __shared__ unsigned long long s_key[4];
    __shared__ uint32_t s_max[4];
    const Geo &g = a.g;
    const int tid = threadIdx.x, b = blockIdx.x, o = blockIdx.y, s = o / a.F, f = o - s * a.F;
    const int32_t *info = a.info + (int64_t)o * 4;
    int32_t *ob = a.blocks + ((int64_t)o * g.nb + b) * 6;
    if (!info[2] || !block_valid(ob, a.min_texture)) return;         // workgroup-uniform; fields 4, 5 are zero already
    const int Dx = OWN ? ob[0] : info[0], Dy = OWN ? ob[1] : info[1];
    const int by = b / g.nbx, bx = b - by * g.nbx;
    const int py = (g.R + 16 * by + 8) * K - P / 2, px = (g.R + 16 * bx + 8) * K - P / 2;         // the patch origin
    unsigned char *tpl = reinterpret_cast<unsigned char *>(s_tpl), *win = reinterpret_cast<unsigned char *>(s_win);
    if (f > 0) {
        for (int i = tid; i < P * P; i += 256) tpl[i] = (unsigned char)src.at(o - 1, py + i / P, px + i % P);
    } else {                                                         // coarse results exist, so the state has been seen
        const uint32_t *sp = reinterpret_cast<const uint32_t *>(a.state + (int64_t)s * a.state_words + ST_HEADER + g.red_bytes / 4) + (int64_t)b * (P * P / 4);
        for (int i = tid; i < P * P / 4; i += 256) s_tpl[i] = sp[i];
    }
    const int wy = py + Dy * K - K, wx = px + Dx * K - K;            // inside the frame by the geometry of the rules
    for (int i = tid; i < WS * WP * 4; i += 256) {
        const int r = i / (WP * 4), c = i - r * (WP * 4);
        win[i] = c < WS ? (unsigned char)src.at(o, wy + r, wx + c) : (unsigned char)0;
    }
    for (int c = tid; c < NCAND; c += 256) s_sad[c] = 0u;
    __syncthreads();
    for (int w = tid; w < NCAND * NPART; w += 256) {
        const int c = w / NPART, part = w - c * NPART;
        const int ey = c / SIDE, ex = c - ey * SIDE;
        atomicAdd(&s_sad[c], sad_rows<BW>(s_tpl, s_win, WP, part * (P / NPART), (part + 1) * (P / NPART), ey, ex));
    }
    __syncthreads();
    unsigned long long best;
    uint32_t smax;
    best_candidate(s_sad, K, s_key, s_max, best, smax);
    if (tid == 0) {
        ob[4] = Dx * K + (int)(best & 63u) - K;
        ob[5] = Dy * K + (int)((best >> 6) & 63u) - K;
    }
}

// 5. workgroups [0, S*F): the frame's result; then SAVE_GROUPS workgroups per stream write the state of its last frame
// FIT (the similarity model): motion_fit_kernel has written the frames' results, only the state is written here
template <int K, typename Src, bool FIT>
__global__ __launch_bounds__(256) void motion_finish_kernel(const Src src, const MotionArgs a) {
    constexpr int P = 8 * K < 32 ? 8 * K : 32;
    __shared__ int s_hist[2 * BINS_MAX];
    __shared__ int s_out[3];
    const Geo &g = a.g;
    const int tid = threadIdx.x, nframes = FIT ? 0 : a.S * a.F;
    if ((int)blockIdx.x < nframes) {
        const int o = blockIdx.x;
        const int32_t *info = a.info + (int64_t)o * 4;
        int32_t *os = a.oshift + (int64_t)o * 4;
        if (!info[2]) {                                              // workgroup-uniform
            if (tid == 0) { os[0] = 0; os[1] = 0; os[2] = 0; os[3] = info[3]; }
            return;
        }
        int dx, dy;
        const int n = block_median(a.blocks + (int64_t)o * g.nb * 6, g.nb, 4, g.R * K + K, a.min_texture, s_hist, s_out, dx, dy);
        if (tid == 0) { os[0] = dx; os[1] = dy; os[2] = 1; os[3] = n; }
        return;
    }
    const int j = (int)blockIdx.x - nframes, s = j / SAVE_GROUPS, part = j - s * SAVE_GROUPS;
    const int o = s * a.F + a.F - 1;
    int32_t *st = a.state + (int64_t)s * a.state_words;
    if (part == 0 && tid < ST_HEADER) st[tid] = tid == 0 ? 1 : 0;
    uint32_t *dred = reinterpret_cast<uint32_t *>(st + ST_HEADER);
    const uint32_t *sred = reinterpret_cast<const uint32_t *>(a.red + (int64_t)o * g.red_bytes);
    const int64_t nred = g.red_bytes / 4, step = (int64_t)SAVE_GROUPS * 256;
    for (int64_t i = (int64_t)part * 256 + tid; i < nred; i += step) dred[i] = sred[i];
    uint32_t *dpat = dred + nred;
    const int64_t npat = g.patch_bytes / 4;                          // four neighbouring pixels of a patch row per item
    for (int64_t i = (int64_t)part * 256 + tid; i < npat; i += step) {
        const int b = (int)(i / (P * P / 4)), r = (int)(i % (P * P / 4));
        const int by = b / g.nbx, bx = b - by * g.nbx;
        const int y = (g.R + 16 * by + 8) * K - P / 2 + r / (P / 4), x = (g.R + 16 * bx + 8) * K - P / 2 + 4 * (r % (P / 4));
        dpat[i] = src.at(o, y, x) | (src.at(o, y, x + 1) << 8) | (src.at(o, y, x + 2) << 16) | (src.at(o, y, x + 3) << 24);
    }
    const int64_t words = a.state_words, used = ST_HEADER + nred + npat;
    if (part == 0 && tid < words - used) st[used + tid] = 0;        // the padding (< 4 words)
}

// ---- the similarity model (include/mydet.h: mydet_motion_warp_frames_rgb_u8) ----
// Everything below is int64.  Bounds, with n <= 1024 blocks, lattice coordinates |u| < 512 (the block lattice: a block's centre
// is (R + 8) k + 16 k u, so the 16 k between lattice steps divides out of the least squares), block vectors |d| <= 136 and
// half-pixel offsets |q| <= 32768: a pair's numerator (dp . dd) << 16 < 2^41; the least-squares numerator
// (m sum(u . d) - sum u . sum d) << 16 < 2^55 and its denominator 16 k (m sum |u|^2 - |sum u|^2) < 2^47; with |a|, |b| < 2^21 (a
// pair's or a fit's |dd| / |dp| <= 272 / 32) the translation's numerator (sum d << 17) - (a sum qx - b sum qy) < 2^48.

__device__ __forceinline__ int64_t floor_div(int64_t num, int64_t den) {                 // den > 0
    const int64_t q = num / den;
    return num - q * den < 0 ? q - 1 : q;
}

__device__ __forceinline__ int64_t isqrt_u64(uint64_t v) {
    uint64_t r = 0, bit = 1ull << 62;
    while (bit > v) bit >>= 2;
    while (bit) {
        if (v >= r + bit) { v -= r + bit; r = (r >> 1) + bit; }
        else r >>= 1;
        bit >>= 2;
    }
    return (int64_t)r;
}

// Q16 degrees of atan(u / 2^16), |u| <= 2^14: the odd polynomial of the header on |u|, constants round(180 / pi / (1, 3, 5, 7) 2^24)
__device__ __forceinline__ int64_t atan_deg_q(int64_t u) {
    const int64_t m = u < 0 ? -u : u, u2 = (m * m) >> 16;
    int64_t p = 137323381;
    p = 192252734 - ((u2 * p) >> 16);
    p = 320421223 - ((u2 * p) >> 16);
    p = 961263669 - ((u2 * p) >> 16);
    const int64_t d = (m * p) >> 24;
    return u < 0 ? -d : d;
}

// The lower median of val[0, n) (n >= 1) by counting: the element whose rank under (value, index) is (n - 1) / 2.  The values
// are complete before the call (a barrier); on return every thread has the median and val may be written again.
__device__ __forceinline__ int64_t rank_median(const int64_t *val, int n, int64_t *res) {
    const int m = (n - 1) / 2;
    for (int i = threadIdx.x; i < n; i += 256) {
        const int64_t vi = val[i];
        int r = 0;
        for (int j = 0; j < n; ++j) {
            const int64_t vj = val[j];
            r += (vj < vi || (vj == vi && j < i)) ? 1 : 0;
        }
        if (r == m) *res = vi;
    }
    __syncthreads();
    return *res;
}

// One workgroup per frame: the fit over the frame's valid blocks -> out_warp, out_shift, the inlier mask.  Every branch around
// a barrier is workgroup-uniform: its condition comes from LDS words every thread reads alike.
__global__ __launch_bounds__(256) void motion_fit_kernel(const MotionArgs a) {
    constexpr int NSUM = 10;
    __shared__ int64_t s_va[NB_MAX], s_vb[NB_MAX];
    __shared__ int s_blk[NB_MAX], s_dx[NB_MAX], s_dy[NB_MAX];
    __shared__ int s_inl[NB_MAX];                                    // by block index
    __shared__ int s_wcnt[NB_MAX / 64];
    __shared__ int64_t s_res[4];
    __shared__ unsigned long long s_sum[NSUM];
    const Geo &g = a.g;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, o = blockIdx.x, nb = g.nb, k = g.k;
    const int32_t *info = a.info + (int64_t)o * 4;
    const int32_t *blk = a.blocks + (int64_t)o * nb * 6;
    int32_t *os = a.oshift + (int64_t)o * 4, *ow = a.owarp + (int64_t)o * 8;
    int32_t *oi = a.oinl ? a.oinl + (int64_t)o * nb : nullptr;
    const int n_valid = info[3];
    bool ok = info[2] != 0;                                          // workgroup-uniform, as every later change of it
    int64_t ma = 0, mb = 0, tx = 0, ty = 0, s_q = 0, deg_q = 0;
    int n = 0, m_in = 0;

    for (int b = tid; b < nb; b += 256) s_inl[b] = 0;
    if (ok) {
        // the valid blocks in ascending block index
        unsigned long long bal[NB_MAX / 256];
#pragma unroll
        for (int c = 0; c < NB_MAX / 256; ++c) {
            const int b = c * 256 + tid;
            bal[c] = __ballot(b < nb && block_valid(blk + (int64_t)b * 6, a.min_texture));
            if (lane == 0) s_wcnt[c * 4 + wave] = __popcll(bal[c]);
        }
        __syncthreads();
#pragma unroll
        for (int c = 0; c < NB_MAX / 256; ++c) {
            const int b = c * 256 + tid;
            int pos = 0;
            for (int i = 0; i < c * 4 + wave; ++i) pos += s_wcnt[i];
            if ((bal[c] >> lane) & 1ull) {
                pos += __popcll(bal[c] & ((1ull << lane) - 1ull));
                s_blk[pos] = b; s_dx[pos] = blk[(int64_t)b * 6 + 4]; s_dy[pos] = blk[(int64_t)b * 6 + 5];
            }
        }
        for (int i = 0; i < NB_MAX / 64; ++i) n += s_wcnt[i];
        __syncthreads();
    }
    const int h = n / 2;
    ok = ok && h > 0;                                                // no pair
    // block i: lattice (ux, uy), centre p, q = 2 p - (W, H)
#define FIT_BLOCK(i)                                                                       \
    const int uy = s_blk[i] / g.nbx, ux = s_blk[i] - uy * g.nbx;                           \
    const int64_t qx = 2 * (int64_t)((g.R + 16 * ux + 8) * k) - g.W, qy = 2 * (int64_t)((g.R + 16 * uy + 8) * k) - g.H; \
    const int64_t dx = s_dx[i], dy = s_dy[i]
    if (ok) {
        for (int i = tid; i < h; i += 256) {
            const int j = i + (n - h);
            const int uyi = s_blk[i] / g.nbx, uxi = s_blk[i] - uyi * g.nbx, uyj = s_blk[j] / g.nbx, uxj = s_blk[j] - uyj * g.nbx;
            const int64_t ex = (int64_t)(16 * k) * (uxj - uxi), ey = (int64_t)(16 * k) * (uyj - uyi);
            const int64_t fx = s_dx[j] - s_dx[i], fy = s_dy[j] - s_dy[i], den = ex * ex + ey * ey;      // > 0: distinct blocks
            s_va[i] = floor_div((ex * fx + ey * fy) << 16, den);
            s_vb[i] = floor_div((ex * fy - ey * fx) << 16, den);
        }
        __syncthreads();
        ma = rank_median(s_va, h, &s_res[0]);
        mb = rank_median(s_vb, h, &s_res[1]);
        for (int i = tid; i < n; i += 256) {
            FIT_BLOCK(i);
            s_va[i] = (dx << 16) - ((ma * qx - mb * qy) >> 1);
            s_vb[i] = (dy << 16) - ((mb * qx + ma * qy) >> 1);
        }
        __syncthreads();
        tx = rank_median(s_va, n, &s_res[2]);
        ty = rank_median(s_vb, n, &s_res[3]);
    }
    for (int round = 0; round < 2; ++round) {
        if (!ok) break;
        if (tid < NSUM) s_sum[tid] = 0ull;
        __syncthreads();
        int64_t acc[NSUM];
#pragma unroll
        for (int q = 0; q < NSUM; ++q) acc[q] = 0;
        for (int i = tid; i < n; i += 256) {
            FIT_BLOCK(i);
            const int64_t rx = (dx << 16) - tx - ((ma * qx - mb * qy) >> 1), ry = (dy << 16) - ty - ((mb * qx + ma * qy) >> 1);
            const bool in = (rx < 0 ? -rx : rx) <= a.tol_q && (ry < 0 ? -ry : ry) <= a.tol_q;
            s_inl[s_blk[i]] = in ? 1 : 0;
            if (in) {
                acc[0] += 1; acc[1] += ux; acc[2] += uy; acc[3] += dx; acc[4] += dy;
                acc[5] += (int64_t)ux * ux + (int64_t)uy * uy;
                acc[6] += ux * dx + uy * dy;
                acc[7] += ux * dy - uy * dx;
                acc[8] += qx; acc[9] += qy;
            }
        }
        if (acc[0]) {
#pragma unroll
            for (int q = 0; q < NSUM; ++q) atomicAdd(&s_sum[q], (unsigned long long)acc[q]);
        }
        __syncthreads();
        const int64_t m = (int64_t)s_sum[0], sux = (int64_t)s_sum[1], suy = (int64_t)s_sum[2], sdx = (int64_t)s_sum[3], sdy = (int64_t)s_sum[4];
        const int64_t suu = (int64_t)s_sum[5], sud = (int64_t)s_sum[6], sxd = (int64_t)s_sum[7], sqx = (int64_t)s_sum[8], sqy = (int64_t)s_sum[9];
        __syncthreads();                                             // s_sum is read: the next round may clear it
        const int64_t den = (int64_t)(16 * k) * (m * suu - (sux * sux + suy * suy));
        if (m < 3 || den == 0) { ok = false; break; }
        ma = floor_div((m * sud - (sux * sdx + suy * sdy)) << 16, den);
        mb = floor_div((m * sxd - (sux * sdy - suy * sdx)) << 16, den);
        tx = floor_div((sdx << 17) - (ma * sqx - mb * sqy), 2 * m);
        ty = floor_div((sdy << 17) - (mb * sqx + ma * sqy), 2 * m);
        m_in = (int)m;
    }
#undef FIT_BLOCK
    if (ok) {                                                        // the derived integers and the caps
        s_q = isqrt_u64((uint64_t)((65536 + ma) * (65536 + ma) + mb * mb));
        const int64_t dz = s_q - 65536;
        ok = (dz < 0 ? -dz : dz) <= a.zoom_q && 65536 + ma > 0;
        ok = ok && (tx < 0 ? -tx : tx) < MOTION_T_LIMIT && (ty < 0 ? -ty : ty) < MOTION_T_LIMIT;
        if (ok) {
            const int64_t u = floor_div(mb << 16, 65536 + ma);
            ok = (u < 0 ? -u : u) <= 16384;
            if (ok) {
                deg_q = atan_deg_q(u);
                ok = (deg_q < 0 ? -deg_q : deg_q) <= a.rot_q;
            }
        }
    }
    __syncthreads();                                                 // s_inl is complete
    if (tid < 8) {
        const int64_t w[8] = {ma, mb, tx, ty, s_q, deg_q, 1, m_in};
        int32_t v = 0;
#pragma unroll
        for (int q = 0; q < 8; ++q) v = tid == q ? (int32_t)w[q] : v;
        ow[tid] = ok ? v : 0;
    }
    if (tid == 0) {
        os[0] = ok ? (int32_t)((tx + 32768) >> 16) : 0; os[1] = ok ? (int32_t)((ty + 32768) >> 16) : 0; os[2] = ok ? 1 : 0; os[3] = n_valid;
    }
    if (oi)
        for (int b = tid; b < nb; b += 256) oi[b] = ok ? s_inl[b] : 0;
}

__global__ __launch_bounds__(256) void motion_reset_kernel(int32_t *state, int64_t words) {
    int32_t *st = state + (int64_t)blockIdx.y * words;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < words; i += (int64_t)gridDim.x * 256) st[i] = 0;
}

template <int K, typename Src>
int motion_launch(const Src &src, const MotionArgs &a, hipStream_t stream) {
    const Geo &g = a.g;
    const unsigned frames = (unsigned)(a.S * a.F);
    hipLaunchKernelGGL((motion_reduce_kernel<K, Src>), dim3((unsigned)((g.hr * (g.wrp / 4) + 255) / 256), frames), dim3(256), 0, stream, src, a);
    hipLaunchKernelGGL(motion_coarse_kernel, dim3((unsigned)g.nb, frames), dim3(256), 0, stream, a);
    hipLaunchKernelGGL(motion_median_kernel, dim3(frames), dim3(256), 0, stream, a);
    if (a.model) {
        hipLaunchKernelGGL((motion_refine_kernel<K, Src, true>), dim3((unsigned)g.nb, frames), dim3(256), 0, stream, src, a);
        hipLaunchKernelGGL(motion_fit_kernel, dim3(frames), dim3(256), 0, stream, a);
        hipLaunchKernelGGL((motion_finish_kernel<K, Src, true>), dim3((unsigned)(a.S * SAVE_GROUPS)), dim3(256), 0, stream, src, a);
        return mydet_launch_status();
    }
    hipLaunchKernelGGL((motion_refine_kernel<K, Src, false>), dim3((unsigned)g.nb, frames), dim3(256), 0, stream, src, a);
    hipLaunchKernelGGL((motion_finish_kernel<K, Src, false>), dim3(frames + (unsigned)(a.S * SAVE_GROUPS)), dim3(256), 0, stream, src, a);
    return mydet_launch_status();
}

template <typename Src>
int motion_launch_k(const Src &src, const MotionArgs &a, hipStream_t stream) {
    if (a.g.k == 2) return motion_launch<2>(src, a, stream);
    if (a.g.k == 4) return motion_launch<4>(src, a, stream);
    return motion_launch<8>(src, a, stream);
}

// The checks both entry points share; fills `a`
int motion_args(MotionArgs &a, int B, int H, int W, int S, const mydet_motion_set *set, int32_t *state, void *ws, int64_t ws_bytes,
                int32_t *out_shift, int32_t *out_blocks, bool warp = false, int32_t *out_warp = nullptr, int32_t *out_inliers = nullptr) {
    a.model = 0; a.tol_q = a.zoom_q = a.rot_q = 0; a.owarp = a.oinl = nullptr;
    if (warp) {                                                      // the similarity model: the reserved words of the settings
        if (!set || !out_warp || ((uintptr_t)out_warp & 3) || ((uintptr_t)out_inliers & 3)) return MYDET_E_BADARG;
        const int *r = set->reserved;
        if (r[0] != MYDET_MOTION_MODEL_SIMILARITY) return MYDET_E_BADARG;
        if (r[1] < 0 || r[1] > 16 << 16 || r[2] < 0 || r[2] > 1 << 14 || r[3] < 0 || r[3] > 14 << 16) return MYDET_E_BADARG;
        a.model = 1;
        a.tol_q = r[1] ? r[1] : 2 << 16; a.zoom_q = r[2] ? r[2] : 1 << 13; a.rot_q = r[3] ? r[3] : 7 << 16;
        a.owarp = out_warp; a.oinl = out_inliers;
    }
    if (B <= 0 || S <= 0 || B % S || !set || !state || !ws || !out_shift) return MYDET_E_BADARG;
    if (((uintptr_t)state & 15) || ((uintptr_t)ws & 15) || ((uintptr_t)out_shift & 3) || ((uintptr_t)out_blocks & 3)) return MYDET_E_BADARG;
    if (H < 1 || W < 1) return MYDET_E_BADARG;
    const int k = set->reduce ? set->reduce : motion_default_reduce(H, W);
    const int st = motion_geo(a.g, H, W, k, set->search);
    if (st) return st;
    if (set->min_texture < 0 || set->min_blocks < 0 || set->min_blocks > NB_MAX) return MYDET_E_BADARG;
    const Ws w = motion_ws(a.g, B);
    if (ws_bytes < w.total) return MYDET_E_BADARG;
    a.S = S; a.F = B / S;
    a.min_texture = set->min_texture;
    a.min_blocks = set->min_blocks ? set->min_blocks : ((a.g.nb + 7) / 8 > 2 ? (a.g.nb + 7) / 8 : 2);
    a.state = state; a.state_words = motion_state_words(a.g);
    a.red = static_cast<unsigned char *>(ws) + w.red;
    a.info = reinterpret_cast<int32_t *>(static_cast<unsigned char *>(ws) + w.info);
    a.blocks = out_blocks ? out_blocks : reinterpret_cast<int32_t *>(static_cast<unsigned char *>(ws) + w.blocks);
    a.oshift = out_shift;
    return 0;
}

}  // namespace

extern "C" int mydet_motion_default_reduce(int H, int W) { return H < 1 || W < 1 ? 0 : motion_default_reduce(H, W); }

extern "C" int64_t mydet_motion_state_words(int H, int W, int k, int R) {
    Geo g;
    return motion_geo(g, H, W, k, R) ? 0 : motion_state_words(g);
}

extern "C" int64_t mydet_motion_workspace_bytes(int frames, int H, int W, int k, int R) {
    Geo g;
    return frames < 1 || motion_geo(g, H, W, k, R) ? 0 : motion_ws(g, frames).total;
}

extern "C" int mydet_motion_reset(int32_t *state, int S, int H, int W, int k, int R, void *stream) {
    if (S <= 0 || !state || ((uintptr_t)state & 15)) return MYDET_E_BADARG;
    Geo g;
    const int st = motion_geo(g, H, W, k, R);
    if (st) return st;
    const int64_t words = motion_state_words(g);
    hipLaunchKernelGGL(motion_reset_kernel, dim3(SAVE_GROUPS, (unsigned)S), dim3(256), 0, (hipStream_t)stream, state, words);
    return mydet_launch_status();
}

extern "C" int mydet_motion_frames_rgb_u8(const unsigned char *src, int B, int H, int W, int64_t img_bytes, int64_t row_bytes, int S,
                                          const mydet_motion_set *set, int32_t *state, void *ws, int64_t ws_bytes, int32_t *out_shift,
                                          int32_t *out_blocks, void *stream) {
    if (!src || img_bytes < 0 || W < 1 || row_bytes < 3 * (int64_t)W) return MYDET_E_BADARG;
    MotionArgs a;
    const int st = motion_args(a, B, H, W, S, set, state, ws, ws_bytes, out_shift, out_blocks);
    if (st) return st;
    const int vec = a.g.k == 2 ? 8 : 16;
    const RgbLuma l = {src, img_bytes, row_bytes, (((uintptr_t)src | (uintptr_t)img_bytes | (uintptr_t)row_bytes) & (uintptr_t)(vec - 1)) ? 0 : 1};
    return motion_launch_k(l, a, (hipStream_t)stream);
}

extern "C" int mydet_motion_warp_frames_rgb_u8(const unsigned char *src, int B, int H, int W, int64_t img_bytes, int64_t row_bytes, int S,
                                               const mydet_motion_set *set, int32_t *state, void *ws, int64_t ws_bytes, int32_t *out_shift,
                                               int32_t *out_warp, int32_t *out_blocks, int32_t *out_inliers, void *stream) {
    if (!src || img_bytes < 0 || W < 1 || row_bytes < 3 * (int64_t)W) return MYDET_E_BADARG;
    MotionArgs a;
    const int st = motion_args(a, B, H, W, S, set, state, ws, ws_bytes, out_shift, out_blocks, true, out_warp, out_inliers);
    if (st) return st;
    const int vec = a.g.k == 2 ? 8 : 16;
    const RgbLuma l = {src, img_bytes, row_bytes, (((uintptr_t)src | (uintptr_t)img_bytes | (uintptr_t)row_bytes) & (uintptr_t)(vec - 1)) ? 0 : 1};
    return motion_launch_k(l, a, (hipStream_t)stream);
}

// The 4:2:0 entry points: warp = false is mydet_motion_frames_yuv420
static int motion_frames_yuv420(const mydet_yuv420_src *src, int B, int H, int W, int S, const mydet_motion_set *set, int32_t *state, void *ws,
                                int64_t ws_bytes, int32_t *out_shift, int32_t *out_blocks, bool warp, int32_t *out_warp,
                                int32_t *out_inliers, void *stream) {
    YuvSrc ys;
    int bps;
    bool planar;
    int st = yuv_source(ys, bps, planar, src, B, H, W);
    if (st) return st;
    MotionArgs a;
    st = motion_args(a, B, H, W, S, set, state, ws, ws_bytes, out_shift, out_blocks, warp, out_warp, out_inliers);
    if (st) return st;
#define MOTION_CALL(BPS, PLANAR)                                                   \
    do {                                                                           \
        const YuvLuma<BPS, PLANAR> l = {ys};                                       \
        return motion_launch_k(l, a, (hipStream_t)stream);                         \
    } while (0)
    YUV_DISPATCH(bps, planar, MOTION_CALL);
#undef MOTION_CALL
    return MYDET_E_BADARG;
}

extern "C" int mydet_motion_warp_frames_yuv420(const mydet_yuv420_src *src, int B, int H, int W, int S, const mydet_motion_set *set,
                                               int32_t *state, void *ws, int64_t ws_bytes, int32_t *out_shift, int32_t *out_warp,
                                               int32_t *out_blocks, int32_t *out_inliers, void *stream) {
    return motion_frames_yuv420(src, B, H, W, S, set, state, ws, ws_bytes, out_shift, out_blocks, true, out_warp, out_inliers, stream);
}

extern "C" int mydet_motion_frames_yuv420(const mydet_yuv420_src *src, int B, int H, int W, int S, const mydet_motion_set *set,
                                          int32_t *state, void *ws, int64_t ws_bytes, int32_t *out_shift, int32_t *out_blocks,
                                          void *stream) {
    return motion_frames_yuv420(src, B, H, W, S, set, state, ws, ws_bytes, out_shift, out_blocks, false, nullptr, nullptr, stream);
}
