// Key frames: the boxes of a key frame's record carried through the frames that follow by their pixels, so that the tracker gets
// one record per frame while the network runs on every n-th (include/mydet.h: mydet_carry_records_rgb_u8 has the rules, DESIGN.md
// section 4 the reasoning; tests/_carry_ref.py restates them in Python integers and every output and the state equal it with ==).
//
// Two launches:
//   1. carry_walk_kernel   one workgroup per (slot, stream) walks the call's F frames in order: the chain is only through the
//                          slot's own position, so slots and streams are parallel.  At a key frame it takes the slot's template
//                          (16 x 16 cell means and, for cells of 2 pixels and more, a 32 x 32 patch) into LDS, where it stays for
//                          the interval; a call that starts inside an interval loads it from the state.  At an in-between frame
//                          the (16 + 2R)^2 window of cell means is built in LDS and searched with the SAD core of the
//                          camera-motion estimator (v_sad_u8 on aligned dwords shifted with v_alignbyte_b32; csrc/motion.hip has
//                          the first copy, whose tests hold it as it is), then the patch refines to single pixels.  It writes
//                          how, offset and sad of its slot, and at the end the slot's state, of which it is the only reader and
//                          writer.  A slot that is empty in the state and below no key frame's count leaves at once.
//   2. carry_emit_kernel   one workgroup per frame: a key frame's row is its key record, copied; an in-between row the alive
//                          slots compacted in key order, their centres moved by the offsets.
#include "common.h"
#include "yuv_fetch.h"

namespace {

constexpr int SLOTS = MYDET_CARRY_SLOTS, SLOT_WORDS = MYDET_CARRY_SLOT_WORDS, SLOT_HEADER = MYDET_CARRY_SLOT_HEADER;
constexpr int R_MAX = 16;                                            // coarse search range and largest cell size
constexpr int CAND_MAX = (2 * R_MAX + 1) * (2 * R_MAX + 1);
constexpr int NPART = 4;                                             // a candidate's rows are summed in four parts
constexpr int KEY_WORDS = 8;                                         // cx, cy, w, h, angle, score, class (2 words)
constexpr int WIN_WORDS = 64 * 17;                                   // the refine window at s = 16; the coarse one is 48 x 13
constexpr int C_LIMIT = 65536;

// ---- the luma of a pixel, per source (the estimator's definition) ----

struct RgbLuma {
    const unsigned char *p;
    int64_t img, row;
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

struct CarryArgs {
    int S, F, K, H, W;
    int every, first, R, min_texture, max_sad;                       // max_sad = 256 max_diff
    int rot, words;                                                  // box_width 5; words of a record
    const int32_t *key;
    int64_t key_stride;
    int32_t *state;
    const int32_t *shift;
    int32_t *ws, *out, *how, *off, *sad;
};

__host__ __device__ __forceinline__ int keys_before(int first, int every, int f) {
    return (first + f + every - 1) / every - (first + every - 1) / every;
}
__device__ __forceinline__ bool is_key(const CarryArgs &a, int f) { return (a.first + f) % a.every == 0; }
__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }

// L at (y, x), clamped to the frame
template <typename Src>
__device__ __forceinline__ uint32_t luma(const Src &src, const CarryArgs &a, int o, int y, int x) {
    return src.at(o, clampi(y, 0, a.H - 1), clampi(x, 0, a.W - 1));
}

// The mean of the s x s cell at (y, x)
template <typename Src>
__device__ __forceinline__ uint32_t cell_mean(const Src &src, const CarryArgs &a, int o, int y, int x, int s) {
    if (s == 1) return luma(src, a, o, y, x);
    uint32_t sum = 0u;
    for (int r = 0; r < s; ++r) {
        const int yy = clampi(y + r, 0, a.H - 1);
        for (int c = 0; c < s; ++c) sum += src.at(o, yy, clampi(x + c, 0, a.W - 1));
    }
    return (sum + (uint32_t)(s * s / 2)) / (uint32_t)(s * s);
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

// The search of one stage over (2 r + 1)^2 candidates whose SADs are complete in s_sad: the smallest key
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

// v16 of rule 1; false when v is not finite or too large
__device__ __forceinline__ bool to_fixed(float v, int &v16) {
    if (!(fabsf(v) < 67108864.0f)) return false;                     // NaN, infinities and |v| >= 2^26
    v16 = (int)floorf(v * 16.0f + 0.5f);
    return true;
}

// 1. one workgroup per (slot, stream).  Every thread holds the slot's scalars; they are workgroup-uniform throughout.
template <typename Src>
__global__ __launch_bounds__(256) void carry_walk_kernel(const Src src, const CarryArgs a) {
    __shared__ uint32_t s_tc[64];                                    // C: 16 rows of 4 dwords
    __shared__ uint32_t s_tp[256];                                   // P: 32 rows of 8 dwords
    __shared__ uint32_t s_win[WIN_WORDS];
    __shared__ uint32_t s_sad[CAND_MAX];
    __shared__ unsigned long long s_key[4];
    __shared__ uint32_t s_max[4];
    const int tid = threadIdx.x, slot = blockIdx.x, s = blockIdx.y;
    int32_t *st = a.state + ((int64_t)s * SLOTS + slot) * SLOT_WORDS;
    const int status0 = st[0];
    int status = status0, cs = 0, cx16 = 0, cy16 = 0, offx = 0, offy = 0, relx = 0, rely = 0;
    int32_t kf[KEY_WORDS] = {0, 0, 0, 0, 0, 0, 0, 0};
    bool tpl_new = false;

    bool wanted = status0 != 0;                                      // below the count of one of the call's key frames, or in the state
    for (int k = 0; k < a.K; ++k) {
        const int cnt = a.key[((int64_t)s * a.K + k) * a.key_stride + MYDET_REC_COUNT];
        wanted = wanted || (cnt >= 1 && cnt <= SLOTS && slot < cnt);
    }
    if (!wanted) {                                                   // workgroup-uniform: its state is zero and stays zero
        for (int i = tid; i < a.F * 5; i += 256) {
            const int f = i / 5, w = i - f * 5;
            const int64_t e = (int64_t)(s * a.F + f) * SLOTS + slot;
            if (w == 0) a.how[e] = 0;
            else if (w < 3) a.off[2 * e + w - 1] = 0;
            else a.sad[2 * e + w - 3] = 0;
        }
        return;
    }
    if (status0 == MYDET_CARRY_HOW_CARRIED) {
        cs = st[1]; cx16 = st[2]; cy16 = st[3]; offx = st[4]; offy = st[5]; relx = st[6]; rely = st[7];
#pragma unroll
        for (int i = 0; i < KEY_WORDS; ++i) kf[i] = st[8 + i];
        if (tid < 64) s_tc[tid] = (uint32_t)st[SLOT_HEADER + tid];
        s_tp[tid] = (uint32_t)st[SLOT_HEADER + 64 + tid];
        if (!is_key(a, 0) && tid < KEY_WORDS) a.ws[((int64_t)s * SLOTS + slot) * KEY_WORDS + tid] = st[8 + tid];
        __syncthreads();
    }

    for (int f = 0; f < a.F; ++f) {
        const int o = s * a.F + f;
        int hw = 0, smin_o = 0, smax_o = 0;
        if (is_key(a, f)) {
            const int32_t *rec = a.key + ((int64_t)s * a.K + keys_before(a.first, a.every, f)) * a.key_stride;
            const int cnt = rec[MYDET_REC_COUNT];
            status = 0; cs = cx16 = cy16 = offx = offy = relx = rely = 0;
#pragma unroll
            for (int i = 0; i < KEY_WORDS; ++i) kf[i] = 0;
            if (cnt >= 1 && cnt <= SLOTS && slot < cnt) {
                hw = MYDET_CARRY_HOW_KEY;
                int32_t b[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) b[i] = rec[MYDET_REC_BBOX + 4 * slot + i];
                int w16 = 0, h16 = 0;
                const bool okx = to_fixed(__int_as_float(b[0]), cx16), oky = to_fixed(__int_as_float(b[1]), cy16);
                const bool okw = to_fixed(__int_as_float(b[2]), w16), okh = to_fixed(__int_as_float(b[3]), h16);
                const bool ok = okx && oky && okw && okh;
                if (ok && w16 > 0 && h16 > 0) {
                    status = MYDET_CARRY_HOW_CARRIED;
                    const int m = w16 < h16 ? w16 : h16, side = a.rot ? m / 2 : (int)(3 * (int64_t)m / 4);
                    cs = clampi((side + 255) / 256, 1, R_MAX);
#pragma unroll
                    for (int i = 0; i < 4; ++i) kf[i] = b[i];
                    kf[4] = a.rot ? rec[MYDET_REC_ANGLE + slot] : 0;
                    kf[5] = rec[MYDET_REC_SCORE + slot];
                    kf[6] = rec[MYDET_REC_CLASS + 2 * slot]; kf[7] = rec[MYDET_REC_CLASS + 2 * slot + 1];
                    const int X = cx16 >> 4, Y = cy16 >> 4;
                    __syncthreads();                                 // the searches of the frame before have read the template
                    reinterpret_cast<unsigned char *>(s_tc)[tid] =
                        (unsigned char)cell_mean(src, a, o, Y - 8 * cs + (tid >> 4) * cs, X - 8 * cs + (tid & 15) * cs, cs);
                    for (int i = tid; i < 1024; i += 256)
                        reinterpret_cast<unsigned char *>(s_tp)[i] = cs >= 2 ? (unsigned char)luma(src, a, o, Y - 16 + (i >> 5), X - 16 + (i & 31)) : (unsigned char)0;
                    tpl_new = true;
                    __syncthreads();
                } else {
                    cx16 = cy16 = 0;
                    status = MYDET_CARRY_HOW_NOT;
                }
            }
        } else if (status == MYDET_CARRY_HOW_CARRIED) {
            int sdx = 0, sdy = 0;
            if (a.shift) {
                const int32_t *q = a.shift + (int64_t)o * 4;
                if (q[2] == 1) { sdx = clampi(q[0], -C_LIMIT, C_LIMIT); sdy = clampi(q[1], -C_LIMIT, C_LIMIT); }
            }
            const int ccx = clampi(offx + relx + sdx, -C_LIMIT, C_LIMIT), ccy = clampi(offy + rely + sdy, -C_LIMIT, C_LIMIT);
            const int R = a.R, side = 2 * R + 1, ncand = side * side, wside = 16 + 2 * R, wp = lds_pitch_dwords(wside);
            const int X = cx16 >> 4, Y = cy16 >> 4;
            const int gy0 = Y - 8 * cs + ccy - R * cs, gx0 = X - 8 * cs + ccx - R * cs;
            unsigned char *win = reinterpret_cast<unsigned char *>(s_win);
            __syncthreads();                                         // the frame before is done with the window and the SADs
            for (int i = tid; i < wside * wp * 4; i += 256) {
                const int r = i / (wp * 4), c = i - r * (wp * 4);
                win[i] = c < wside ? (unsigned char)cell_mean(src, a, o, gy0 + r * cs, gx0 + c * cs, cs) : (unsigned char)0;
            }
            for (int c = tid; c < ncand; c += 256) s_sad[c] = 0u;
            __syncthreads();
            for (int w = tid; w < ncand * NPART; w += 256) {
                const int c = w / NPART, part = w - c * NPART;
                const int dy = c / side, dx = c - dy * side;         // offsets from the window's origin: (dy - R) + R
                atomicAdd(&s_sad[c], sad_rows<4>(s_tc, s_win, wp, 4 * part, 4 * part + 4, dy, dx));
            }
            __syncthreads();
            unsigned long long best;
            uint32_t smax;
            best_candidate(s_sad, R, s_key, s_max, best, smax);
            const int smin = (int)(best >> 24);
            smin_o = smin; smax_o = (int)smax;
            if ((int)smax - smin < a.min_texture) {
                status = MYDET_CARRY_HOW_FLAT;
            } else if (smin > a.max_sad) {
                status = MYDET_CARRY_HOW_LOST;
            } else {
                int nx = ccx + ((int)(best & 63u) - R) * cs, ny = ccy + ((int)((best >> 6) & 63u) - R) * cs;
                if (cs >= 2) {
                    const int ws2 = 32 + 2 * cs, wp2 = lds_pitch_dwords(ws2), side2 = 2 * cs + 1, ncand2 = side2 * side2;
                    const int py0 = Y - 16 + ny - cs, px0 = X - 16 + nx - cs;
                    __syncthreads();                                 // everyone has its coarse result
                    for (int i = tid; i < ws2 * wp2 * 4; i += 256) {
                        const int r = i / (wp2 * 4), c = i - r * (wp2 * 4);
                        win[i] = c < ws2 ? (unsigned char)luma(src, a, o, py0 + r, px0 + c) : (unsigned char)0;
                    }
                    for (int c = tid; c < ncand2; c += 256) s_sad[c] = 0u;
                    __syncthreads();
                    for (int w = tid; w < ncand2 * NPART; w += 256) {
                        const int c = w / NPART, part = w - c * NPART;
                        const int ey = c / side2, ex = c - ey * side2;
                        atomicAdd(&s_sad[c], sad_rows<8>(s_tp, s_win, wp2, 8 * part, 8 * part + 8, ey, ex));
                    }
                    __syncthreads();
                    unsigned long long best2;
                    uint32_t smax2;
                    best_candidate(s_sad, cs, s_key, s_max, best2, smax2);
                    nx += (int)(best2 & 63u) - cs;
                    ny += (int)((best2 >> 6) & 63u) - cs;
                }
                relx = (nx - offx) - sdx; rely = (ny - offy) - sdy;
                offx = nx; offy = ny;
                const int px = X + offx, py = Y + offy;
                if (px < 0 || px >= a.W || py < 0 || py >= a.H) status = MYDET_CARRY_HOW_LEFT;
            }
            hw = status;
        } else {
            hw = status;
        }
        if (tid == 0) {
            const int64_t e = (int64_t)o * SLOTS + slot;
            const bool alive = hw == MYDET_CARRY_HOW_CARRIED;
            a.how[e] = hw;
            a.off[2 * e] = alive ? offx : 0; a.off[2 * e + 1] = alive ? offy : 0;
            a.sad[2 * e] = smin_o; a.sad[2 * e + 1] = smax_o;
        }
    }

    // the slot's state: every word but the status is zero unless the slot is alive
    const bool alive = status == MYDET_CARRY_HOW_CARRIED;
    if (tid < SLOT_HEADER) {
        int32_t v = 0;
        if (tid == 0) {
            v = status;
        } else if (alive) {                                          // selects, not an indexed array: the scalars stay in registers
            v = tid == 1 ? cs : tid == 2 ? cx16 : tid == 3 ? cy16 : tid == 4 ? offx : tid == 5 ? offy : tid == 6 ? relx : rely;
#pragma unroll
            for (int i = 0; i < KEY_WORDS; ++i)
                if (tid == 8 + i) v = kf[i];
        }
        st[tid] = v;
    }
    if (alive && tpl_new) {
        __syncthreads();
        if (tid < 64) st[SLOT_HEADER + tid] = (int32_t)s_tc[tid];
        st[SLOT_HEADER + 64 + tid] = (int32_t)s_tp[tid];
    } else if (!alive && status0 == MYDET_CARRY_HOW_CARRIED) {
        for (int i = tid; i < SLOT_WORDS - SLOT_HEADER; i += 256) st[SLOT_HEADER + i] = 0;
    }
}

// 2. one workgroup per frame
__global__ __launch_bounds__(256) void carry_emit_kernel(const CarryArgs a) {
    __shared__ int s_tot[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int o = blockIdx.x, s = o / a.F, f = o - s * a.F;
    int32_t *out = a.out + (int64_t)o * a.words;
    const int nb = keys_before(a.first, a.every, f);
    if (is_key(a, f)) {                                              // workgroup-uniform
        const int32_t *rec = a.key + ((int64_t)s * a.K + nb) * a.key_stride;
        for (int i = tid; i < a.words; i += 256) out[i] = rec[i];
        return;
    }
    const int32_t *how = a.how + (int64_t)o * SLOTS;
    const int j0 = 2 * tid;
    const int a0 = how[j0] == MYDET_CARRY_HOW_CARRIED, a1 = how[j0 + 1] == MYDET_CARRY_HOW_CARRIED;
    int incl = a0 + a1;                                              // the inclusive prefix sum over the threads, in slot order
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int v = __shfl_up(incl, d, 64);
        if (lane >= d) incl += v;
    }
    if (lane == 63) s_tot[wave] = incl;
    __syncthreads();
    int base = incl - (a0 + a1), total = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        if (w < wave) base += s_tot[w];
        total += s_tot[w];
    }
    const int32_t *rec = nb > 0 ? a.key + ((int64_t)s * a.K + nb - 1) * a.key_stride : nullptr;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        if (!(h ? a1 : a0)) continue;
        const int j = j0 + h, d = base + (h ? a0 : 0);
        int32_t kf[KEY_WORDS];
        if (rec) {
#pragma unroll
            for (int i = 0; i < 4; ++i) kf[i] = rec[MYDET_REC_BBOX + 4 * j + i];
            kf[4] = a.rot ? rec[MYDET_REC_ANGLE + j] : 0;
            kf[5] = rec[MYDET_REC_SCORE + j];
            kf[6] = rec[MYDET_REC_CLASS + 2 * j]; kf[7] = rec[MYDET_REC_CLASS + 2 * j + 1];
        } else {
            const int32_t *q = a.ws + ((int64_t)s * SLOTS + j) * KEY_WORDS;
#pragma unroll
            for (int i = 0; i < KEY_WORDS; ++i) kf[i] = q[i];
        }
        const int32_t *of = a.off + ((int64_t)o * SLOTS + j) * 2;
        out[MYDET_REC_BBOX + 4 * d] = __float_as_int(__int_as_float(kf[0]) + (float)of[0]);
        out[MYDET_REC_BBOX + 4 * d + 1] = __float_as_int(__int_as_float(kf[1]) + (float)of[1]);
        out[MYDET_REC_BBOX + 4 * d + 2] = kf[2];
        out[MYDET_REC_BBOX + 4 * d + 3] = kf[3];
        out[MYDET_REC_SCORE + d] = kf[5];
        out[MYDET_REC_CLASS + 2 * d] = kf[6]; out[MYDET_REC_CLASS + 2 * d + 1] = kf[7];
        out[MYDET_REC_INDEX + d] = j;
        if (a.rot) out[MYDET_REC_ANGLE + d] = kf[4];
    }
    if (tid < 4) out[tid] = tid == 0 ? total : 0;
    for (int d = total + tid; d < SLOTS; d += 256) {                 // entries from COUNT on are zero
#pragma unroll
        for (int i = 0; i < 4; ++i) out[MYDET_REC_BBOX + 4 * d + i] = 0;
        out[MYDET_REC_SCORE + d] = 0;
        out[MYDET_REC_CLASS + 2 * d] = 0; out[MYDET_REC_CLASS + 2 * d + 1] = 0;
        out[MYDET_REC_INDEX + d] = 0;
        if (a.rot) out[MYDET_REC_ANGLE + d] = 0;
    }
}

__global__ __launch_bounds__(256) void carry_reset_kernel(int32_t *state, int64_t words) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < words; i += (int64_t)gridDim.x * 256) state[i] = 0;
}

template <typename Src>
int carry_launch(const Src &src, const CarryArgs &a, hipStream_t stream) {
    hipLaunchKernelGGL((carry_walk_kernel<Src>), dim3(SLOTS, (unsigned)a.S), dim3(256), 0, stream, src, a);
    hipLaunchKernelGGL(carry_emit_kernel, dim3((unsigned)(a.S * a.F)), dim3(256), 0, stream, a);
    return mydet_launch_status();
}

// The checks both entry points share; fills `a`
int carry_args(CarryArgs &a, int B, int H, int W, int S, const mydet_carry_set *set, int first, const int32_t *key_records,
               int64_t key_stride_words, int box_width, int32_t *state, const int32_t *shift, int32_t *ws, int32_t *out_records,
               int32_t *out_how, int32_t *out_offset, int32_t *out_sad) {
    if (B <= 0 || S <= 0 || S > 65535 || B % S || !set) return MYDET_E_BADARG;
    if (H < 1 || W < 1 || H > MYDET_ZONE_MAX_FRAME || W > MYDET_ZONE_MAX_FRAME) return MYDET_E_BADARG;
    if (set->every < 1 || set->every > MYDET_CARRY_MAX_EVERY || set->search < 4 || set->search > R_MAX) return MYDET_E_BADARG;
    if (set->min_texture < 0 || set->min_texture >= 1 << 24 || set->max_diff < 0 || set->max_diff > 255) return MYDET_E_BADARG;
    if (first < 0 || first >= set->every || (box_width != 4 && box_width != 5)) return MYDET_E_BADARG;
    a.words = box_width == 4 ? MYDET_REC_WORDS : MYDET_REC_ROT_WORDS;
    a.S = S; a.F = B / S; a.K = keys_before(first, set->every, a.F);
    if (!state || !ws || !out_records || !out_how || !out_offset || !out_sad || (a.K > 0 && !key_records)) return MYDET_E_BADARG;
    if (((uintptr_t)state & 15) || ((uintptr_t)out_records & 15) || ((uintptr_t)key_records & 15)) return MYDET_E_BADARG;
    if (((uintptr_t)ws | (uintptr_t)out_how | (uintptr_t)out_offset | (uintptr_t)out_sad | (uintptr_t)shift) & 3) return MYDET_E_BADARG;
    if (a.K > 0 && (key_stride_words < a.words || key_stride_words % 4)) return MYDET_E_BADARG;
    a.H = H; a.W = W;
    a.every = set->every; a.first = first; a.R = set->search; a.min_texture = set->min_texture; a.max_sad = 256 * set->max_diff;
    a.rot = box_width == 5;
    a.key = key_records; a.key_stride = key_stride_words;
    a.state = state; a.shift = shift; a.ws = ws; a.out = out_records; a.how = out_how; a.off = out_offset; a.sad = out_sad;
    return 0;
}

}  // namespace

extern "C" int64_t mydet_carry_state_words(void) { return (int64_t)SLOTS * SLOT_WORDS; }

extern "C" int mydet_carry_reset(int32_t *state, int S, void *stream) {
    if (S <= 0 || !state || ((uintptr_t)state & 15)) return MYDET_E_BADARG;
    const int64_t words = (int64_t)S * SLOTS * SLOT_WORDS;
    hipLaunchKernelGGL(carry_reset_kernel, dim3(grid_for(words)), dim3(256), 0, (hipStream_t)stream, state, words);
    return mydet_launch_status();
}

extern "C" int mydet_carry_records_rgb_u8(const unsigned char *src, int B, int H, int W, int64_t img_bytes, int64_t row_bytes, int S,
                                          const mydet_carry_set *set, int first, const int32_t *key_records, int64_t key_stride_words,
                                          int box_width, int32_t *state, const int32_t *shift, int32_t *ws, int32_t *out_records,
                                          int32_t *out_how, int32_t *out_offset, int32_t *out_sad, void *stream) {
    if (!src || img_bytes < 0 || W < 1 || row_bytes < 3 * (int64_t)W) return MYDET_E_BADARG;
    CarryArgs a;
    const int st = carry_args(a, B, H, W, S, set, first, key_records, key_stride_words, box_width, state, shift, ws, out_records, out_how,
                              out_offset, out_sad);
    if (st) return st;
    const RgbLuma l = {src, img_bytes, row_bytes};
    return carry_launch(l, a, (hipStream_t)stream);
}

extern "C" int mydet_carry_records_yuv420(const mydet_yuv420_src *src, int B, int H, int W, int S, const mydet_carry_set *set, int first,
                                          const int32_t *key_records, int64_t key_stride_words, int box_width, int32_t *state,
                                          const int32_t *shift, int32_t *ws, int32_t *out_records, int32_t *out_how, int32_t *out_offset,
                                          int32_t *out_sad, void *stream) {
    YuvSrc ys;
    int bps;
    bool planar;
    int st = yuv_source(ys, bps, planar, src, B, H, W);
    if (st) return st;
    CarryArgs a;
    st = carry_args(a, B, H, W, S, set, first, key_records, key_stride_words, box_width, state, shift, ws, out_records, out_how, out_offset,
                    out_sad);
    if (st) return st;
#define CARRY_CALL(BPS, PLANAR)                                                    \
    do {                                                                           \
        const YuvLuma<BPS, PLANAR> l = {ys};                                       \
        return carry_launch(l, a, (hipStream_t)stream);                            \
    } while (0)
    YUV_DISPATCH(bps, planar, CARRY_CALL);
#undef CARRY_CALL
    return MYDET_E_BADARG;
}
