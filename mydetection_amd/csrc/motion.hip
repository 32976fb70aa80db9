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
template <int K, typename Src>
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
    const int Dx = info[0], Dy = info[1];
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
template <int K, typename Src>
__global__ __launch_bounds__(256) void motion_finish_kernel(const Src src, const MotionArgs a) {
    constexpr int P = 8 * K < 32 ? 8 * K : 32;
    __shared__ int s_hist[2 * BINS_MAX];
    __shared__ int s_out[3];
    const Geo &g = a.g;
    const int tid = threadIdx.x, nframes = a.S * a.F;
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
    hipLaunchKernelGGL((motion_refine_kernel<K, Src>), dim3((unsigned)g.nb, frames), dim3(256), 0, stream, src, a);
    hipLaunchKernelGGL((motion_finish_kernel<K, Src>), dim3(frames + (unsigned)(a.S * SAVE_GROUPS)), dim3(256), 0, stream, src, a);
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
                int32_t *out_shift, int32_t *out_blocks) {
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

extern "C" int mydet_motion_frames_yuv420(const mydet_yuv420_src *src, int B, int H, int W, int S, const mydet_motion_set *set,
                                          int32_t *state, void *ws, int64_t ws_bytes, int32_t *out_shift, int32_t *out_blocks,
                                          void *stream) {
    YuvSrc ys;
    int bps;
    bool planar;
    int st = yuv_source(ys, bps, planar, src, B, H, W);
    if (st) return st;
    MotionArgs a;
    st = motion_args(a, B, H, W, S, set, state, ws, ws_bytes, out_shift, out_blocks);
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
