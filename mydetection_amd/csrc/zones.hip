// Counting tracks in zones and across lines on the device: the launch behind the tracker launch (include/mydet.h:
// mydet_zones_frames has the rules, DESIGN.md section 4 the reasoning; tests/_zones_ref.py restates them in Python).
//
// One workgroup per stream, thread = track slot, as track_kernel: a track keeps its slot for life, so the slot's zone state --
// the id it belongs to, the zone bits, the remembered side of every line, the previous anchor, the frame it entered each zone --
// lives in its thread's registers for all F frames of the launch.  The quantised polygons and lines are staged once in LDS from
// the parameter struct; every read of them is one address for the whole wave (a broadcast).  A polygon is staged as edge records:
// the edge turned so that d = b.y - a.y > 0 (the rule gives the same answer for (a, b) and (b, a)), with the rule's inequality
// (p.x - a.x) * d < (b.x - a.x) * (p.y - a.y) moved to p.x * d - p.y * dx < a.x * d - dx * a.y, whose right side is a constant of
// the edge -- the same integers, no overflow (|products| <= 2^42).  The test of an edge is then two compares, two 64-bit
// multiply-adds and a 64-bit compare, without a branch, and the records are read four edges at a time, so the LDS latency is paid
// once per four edges and not, with a divergent branch, once per edge (measured: profiles/zones.md).  Per frame each thread reads its own
// id / missed / cls / box, decides with integer comparisons (products of two int32 values in int64), and the frame's events
// are counted by ballot and popcount: lane k of a wave ends up holding the wave's count for zone k (occupancy, entries, exits,
// lost) or crossing bit k, the waves' counts meet in LDS (double-buffered: one barrier per frame), and thread z < 16 owns the
// cumulative counters of zone z, thread 16 + j those of crossing bit j, in registers.  Dwell sums and maxima are rare events and
// take LDS atomics (integers: the order does not matter); heat cells take global atomics.  Every barrier is on workgroup-uniform
// control flow: the bad-class test reads one word per frame, the same for every thread.
#include "common.h"

namespace {

constexpr int ZMAX = MYDET_ZONES_MAX, VMAX = MYDET_ZONE_MAX_VERTICES;
constexpr int TMAX = MYDET_TRACK_MAX_TRACKS, NWMAX = TMAX / 64;
constexpr int P_OCC = 0, P_ENT = ZMAX, P_EXIT = 2 * ZMAX, P_LOST = 3 * ZMAX, P_CROSS = 4 * ZMAX, NPART = 6 * ZMAX;
// the header of the state (include/mydet.h), in words
constexpr int ST_NOW = 0, ST_ZC = 4, ST_LC = ST_ZC + 4 * ZMAX, ST_DMAX = ST_LC + 2 * ZMAX, ST_DSUM = ST_DMAX + ZMAX;
static_assert(ST_DSUM + 2 * ZMAX == MYDET_ZONES_STATE_HEADER && ST_DSUM % 2 == 0, "the header of include/mydet.h");
static_assert(2 + 4 + ZMAX == MYDET_ZONES_SLOT_WORDS, "the slot planes of include/mydet.h");
static_assert(2 * ZMAX <= 32 && 3 * ZMAX <= 64, "one bit per crossing direction; the owners of the counters fit one wavefront");

struct ZoneArgs {
    const float *box;
    const int64_t *id, *cls;
    const int32_t *missed, *count;
    int F, MT;
    int32_t *state;
    int64_t state_words;              // per stream
    int32_t *heat;
    int32_t *oinside, *ocrossed, *odwell, *oocc, *ozc, *olc;
    mydet_zone_set zs;
};

__device__ __forceinline__ bool zone_finite(float v) { return v - v == 0.0f; }

__device__ __forceinline__ int zone_q(float v) { return (int)floorf(fminf(fmaxf(v * 16.0f, -1048576.0f), 1048576.0f)); }

__device__ __forceinline__ int64_t zone_cross(int ux, int uy, int vx, int vy) { return (int64_t)ux * vy - (int64_t)uy * vx; }

__device__ __forceinline__ int zone_sign(int64_t c) { return c > 0 ? 1 : c < 0 ? -1 : 0; }

// An edge as the inside test reads it: a.y <= b.y; d = b.y - a.y, dx = b.x - a.x; c = a.x * d - dx * a.y.  A horizontal edge
// (and the padding up to a multiple of EDGE_STEP edges: all zero) never straddles a row, whatever its other fields.
typedef int i32x4 __attribute__((ext_vector_type(4)));             // ay, by, d, dx
constexpr int EDGE_STEP = 4;
static_assert(VMAX % EDGE_STEP == 0, "a polygon's records are read EDGE_STEP at a time");

// even-odd, half-open (include/mydet.h); the toggles commute, so the order of the edges does not matter
__device__ __forceinline__ bool zone_inside(const i32x4 *edge, const int64_t *ec, int n, int px, int py) {
    bool in = false;
    for (int e0 = 0; e0 < n; e0 += EDGE_STEP) {
#pragma unroll
        for (int e = e0; e < e0 + EDGE_STEP; ++e) {
            const i32x4 r = edge[e];
            const int64_t t = (int64_t)px * r.z - (int64_t)py * r.w;
            in ^= (r.x <= py) & (py < r.y) & (t < ec[e]);
        }
    }
    return in;
}

__global__ __launch_bounds__(TMAX) void zones_kernel(const ZoneArgs a) {
    __shared__ i32x4 s_edge[ZMAX][VMAX];
    __shared__ int64_t s_edgec[ZMAX][VMAX];
    __shared__ int s_nv[ZMAX];
    __shared__ i32x4 s_line[ZMAX];                                  // A.x, A.y, B.x, B.y
    __shared__ int s_part[2][NWMAX][NPART];
    __shared__ unsigned long long s_dsum[ZMAX];
    __shared__ int s_dmax[ZMAX];

    const int tid = threadIdx.x, nthr = blockDim.x, lane = tid & 63, wave = tid >> 6, nwave = nthr >> 6;
    const int s = blockIdx.x, MT = a.MT, F = a.F;
    const int nz = a.zs.n_polygons, nl = a.zs.n_lines, ncls = a.zs.n_classes;
    const bool bottom = a.zs.anchor == MYDET_ZONE_ANCHOR_BOTTOM, coasting = a.zs.coasting != 0;
    const int gh = a.zs.heat_h, gw = a.zs.heat_w, lim_x = 16 * a.zs.img_w, lim_y = 16 * a.zs.img_h;

    // state views (include/mydet.h: the layout is public)
    int32_t *st = a.state + (int64_t)s * a.state_words;
    int64_t *g_id = reinterpret_cast<int64_t *>(st + MYDET_ZONES_STATE_HEADER);
    int32_t *g_inside = reinterpret_cast<int32_t *>(g_id + MT);
    int32_t *g_sides = g_inside + MT, *g_px = g_sides + MT, *g_py = g_px + MT, *g_ent = g_py + MT;

    for (int i = tid; i < ZMAX * VMAX; i += nthr) {
        const int z = i / VMAX, e = i % VMAX, n = a.zs.n_vertices[z];
        i32x4 r = {0, 0, 0, 0};
        int64_t c = 0;
        if (z < nz && e < n) {
            const int e1 = e + 1 == n ? 0 : e + 1;
            int ax = a.zs.polygon[z][e][0], ay = a.zs.polygon[z][e][1], bx = a.zs.polygon[z][e1][0], by = a.zs.polygon[z][e1][1];
            if (by < ay) { const int tx = ax, ty = ay; ax = bx; ay = by; bx = tx; by = ty; }
            const int d = by - ay, dx = bx - ax;
            r = i32x4{ay, by, d, dx};
            c = (int64_t)ax * d - (int64_t)dx * ay;
        }
        s_edge[z][e] = r;
        s_edgec[z][e] = c;
    }
    for (int i = tid; i < ZMAX; i += nthr) s_line[i] = i32x4{a.zs.line[i][0], a.zs.line[i][1], a.zs.line[i][2], a.zs.line[i][3]};
    if (tid < ZMAX) {
        s_nv[tid] = a.zs.n_vertices[tid];
        s_dsum[tid] = reinterpret_cast<const unsigned long long *>(st + ST_DSUM)[tid];
        s_dmax[tid] = st[ST_DMAX + tid];
    }

    const bool slot_ok = tid < MT;
    int64_t sid = 0;
    unsigned inside = 0u, sides = 0u;
    int ppx = 0, ppy = 0, ent[ZMAX];
#pragma unroll
    for (int z = 0; z < ZMAX; ++z) ent[z] = 0;
    if (slot_ok) {
        sid = g_id[tid]; inside = (unsigned)g_inside[tid]; sides = (unsigned)g_sides[tid]; ppx = g_px[tid]; ppy = g_py[tid];
#pragma unroll
        for (int z = 0; z < ZMAX; ++z) ent[z] = g_ent[z * MT + tid];
    }
    // the cumulative counters: thread z < 16 owns zone z, thread 16 + j crossing bit j (line j / 2, positive first)
    int zc0 = 0, zc1 = 0, zc2 = 0, zc3 = 0, lc = 0;
    if (tid < ZMAX) { zc0 = st[ST_ZC + 4 * tid]; zc1 = st[ST_ZC + 4 * tid + 1]; zc2 = st[ST_ZC + 4 * tid + 2]; zc3 = st[ST_ZC + 4 * tid + 3]; }
    if (tid >= ZMAX && tid < 3 * ZMAX) lc = st[ST_LC + tid - ZMAX];
    int now = st[ST_NOW];
    __syncthreads();                                               // the zone set and the dwell accumulators are in LDS

    for (int f = 0; f < F; ++f) {
        const int64_t o = (int64_t)s * F + f;
        const bool bad = a.count[o] < 0;                           // workgroup-uniform
        unsigned ev_ent = 0u, ev_exit = 0u, ev_lost = 0u, crossed = 0u, shown = 0u;
        if (slot_ok && !bad) {
            const int64_t at = o * MT + tid;
            const int64_t id = a.id[at];
            // 2. close
            if (sid != 0 && sid != id) {
                ev_lost = inside;
#pragma unroll
                for (int z = 0; z < ZMAX; ++z) {
                    if ((inside >> z) & 1u) {
                        const int d = now - ent[z];
                        atomicAdd(&s_dsum[z], (unsigned long long)(long long)d);
                        atomicMax(&s_dmax[z], d);
                    }
                    ent[z] = 0;
                }
                sid = 0; inside = 0u; sides = 0u; ppx = 0; ppy = 0;
            }
            // 3. observe
            if (id != 0) {
                const int ms = a.missed[at];
                bool obs = ms == 0 || (coasting && ms > 0);
                if (obs && ncls > 0) {
                    const int64_t c = a.cls[at];
                    bool pass = false;
                    for (int i = 0; i < ncls; ++i) pass = pass || c == (int64_t)a.zs.classes[i];
                    obs = pass;
                }
                float fx = 0.0f, fy = 0.0f;
                if (obs) {
                    const float *b = a.box + at * 5;
                    fx = b[0];
                    fy = bottom ? b[1] + b[3] / 2.0f : b[1];
                    obs = zone_finite(fx) && zone_finite(fy);
                }
                if (obs) {
                    const int px = zone_q(fx), py = zone_q(fy);
                    if (sid == 0) sid = id;
                    unsigned in_now = 0u;
                    for (int z = 0; z < nz; ++z) in_now |= (zone_inside(s_edge[z], s_edgec[z], s_nv[z], px, py) ? 1u : 0u) << z;
                    ev_ent = in_now & ~inside;
                    ev_exit = inside & ~in_now;
#pragma unroll
                    for (int z = 0; z < ZMAX; ++z) {
                        if ((ev_exit >> z) & 1u) {
                            const int d = now - ent[z];
                            atomicAdd(&s_dsum[z], (unsigned long long)(long long)d);
                            atomicMax(&s_dmax[z], d);
                            ent[z] = 0;
                        }
                        if ((ev_ent >> z) & 1u) ent[z] = now;
                    }
                    inside = in_now;
                    for (int l = 0; l < nl; ++l) {
                        const i32x4 ab = s_line[l];
                        const int ax = ab.x, ay = ab.y, bx = ab.z, by = ab.w;
                        const int sg = zone_sign(zone_cross(bx - ax, by - ay, px - ax, py - ay));
                        if (sg != 0) {
                            const unsigned code = sg > 0 ? 1u : 2u, prev = (sides >> (2 * l)) & 3u;
                            if (prev != 0u && prev != code) {
                                const int ux = px - ppx, uy = py - ppy;
                                const int s1 = zone_sign(zone_cross(ux, uy, ax - ppx, ay - ppy));
                                const int s2 = zone_sign(zone_cross(ux, uy, bx - ppx, by - ppy));
                                if (s1 * s2 <= 0) crossed |= 1u << (2 * l + (sg > 0 ? 0 : 1));
                            }
                            sides = (sides & ~(3u << (2 * l))) | (code << (2 * l));
                        }
                    }
                    ppx = px; ppy = py;
                    // 5. heat
                    if (gh > 0 && ms == 0 && px >= 0 && px < lim_x && py >= 0 && py < lim_y) {
                        const int cy = py * gh / lim_y, cx = px * gw / lim_x;
                        atomicAdd(a.heat + ((int64_t)s * gh + cy) * gw + cx, 1);
                    }
                }
            }
            if (sid == id) shown = inside;
        }
        // 4. the slot's outputs
        if (slot_ok) {
            const int64_t at = o * MT + tid;
            a.oinside[at] = (int)shown;
            a.ocrossed[at] = (int)crossed;
            int32_t *od = a.odwell + at * nz;
#pragma unroll
            for (int z = 0; z < ZMAX; ++z)
                if (z < nz) od[z] = ((shown >> z) & 1u) ? now - ent[z] : -1;
        }
        // the wave's counts: lane k takes zone k and crossing bit k
        int c_occ = 0, c_ent = 0, c_exit = 0, c_lost = 0, c_cross = 0;
        for (int z = 0; z < nz; ++z) {
            const int n_occ = __popcll(__ballot((inside >> z) & 1u)), n_ent = __popcll(__ballot((ev_ent >> z) & 1u));
            const int n_exit = __popcll(__ballot((ev_exit >> z) & 1u)), n_lost = __popcll(__ballot((ev_lost >> z) & 1u));
            if (lane == z) { c_occ = n_occ; c_ent = n_ent; c_exit = n_exit; c_lost = n_lost; }
        }
        for (int k = 0; k < 2 * nl; ++k) {
            const int n_cross = __popcll(__ballot((crossed >> k) & 1u));
            if (lane == k) c_cross = n_cross;
        }
        int *part = s_part[f & 1][wave];
        if (lane < ZMAX) { part[P_OCC + lane] = c_occ; part[P_ENT + lane] = c_ent; part[P_EXIT + lane] = c_exit; part[P_LOST + lane] = c_lost; }
        if (lane < 2 * ZMAX) part[P_CROSS + lane] = c_cross;
        __syncthreads();                                           // the one barrier of the frame (s_part is double-buffered)
        if (tid < ZMAX) {
            int occ = 0;
            for (int w = 0; w < nwave; ++w) {
                const int *p = s_part[f & 1][w];
                occ += p[P_OCC + tid];
                const int e = p[P_ENT + tid], x = p[P_EXIT + tid], l = p[P_LOST + tid];
                zc0 += e; zc1 += x; zc2 += l; zc3 += x + l;
            }
            if (tid < nz) {
                a.oocc[o * nz + tid] = occ;
                int32_t *r = a.ozc + (o * nz + tid) * 4;
                r[0] = zc0; r[1] = zc1; r[2] = zc2; r[3] = zc3;
            }
        } else if (tid < 3 * ZMAX) {
            const int j = tid - ZMAX;
            for (int w = 0; w < nwave; ++w) lc += s_part[f & 1][w][P_CROSS + j];
            if (j < 2 * nl) a.olc[o * (2 * nl) + j] = lc;
        }
        now += 1;                                                  // 6.
    }

    if (slot_ok) {
        g_id[tid] = sid; g_inside[tid] = (int)inside; g_sides[tid] = (int)sides; g_px[tid] = ppx; g_py[tid] = ppy;
#pragma unroll
        for (int z = 0; z < ZMAX; ++z) g_ent[z * MT + tid] = ent[z];
    }
    // every dwell atomic precedes the last frame's barrier
    if (tid < ZMAX) {
        st[ST_ZC + 4 * tid] = zc0; st[ST_ZC + 4 * tid + 1] = zc1; st[ST_ZC + 4 * tid + 2] = zc2; st[ST_ZC + 4 * tid + 3] = zc3;
        st[ST_DMAX + tid] = s_dmax[tid];
        reinterpret_cast<unsigned long long *>(st + ST_DSUM)[tid] = s_dsum[tid];
    } else if (tid < 3 * ZMAX) {
        st[ST_LC + tid - ZMAX] = lc;
    }
    if (tid == 0) st[ST_NOW] = now;
}

__global__ __launch_bounds__(256) void zones_reset_kernel(int32_t *state, int64_t words) {
    int32_t *st = state + (int64_t)blockIdx.x * words;
    for (int64_t i = threadIdx.x; i < words; i += 256) st[i] = 0;
}

inline bool zone_coord_ok(int v) { return v >= -MYDET_ZONE_COORD_MAX && v <= MYDET_ZONE_COORD_MAX; }

bool zone_set_ok(const mydet_zone_set &z) {
    if (z.n_polygons < 0 || z.n_polygons > MYDET_ZONES_MAX || z.n_lines < 0 || z.n_lines > MYDET_ZONES_MAX) return false;
    if (z.n_polygons == 0 && z.n_lines == 0) return false;
    if (z.n_classes < 0 || z.n_classes > MYDET_ZONE_MAX_CLASSES) return false;
    if (z.anchor != MYDET_ZONE_ANCHOR_CENTER && z.anchor != MYDET_ZONE_ANCHOR_BOTTOM) return false;
    if (z.coasting != 0 && z.coasting != 1) return false;
    if (z.img_h < 1 || z.img_h > MYDET_ZONE_MAX_FRAME || z.img_w < 1 || z.img_w > MYDET_ZONE_MAX_FRAME) return false;
    if ((z.heat_h == 0) != (z.heat_w == 0)) return false;
    if (z.heat_h < 0 || z.heat_h > MYDET_ZONE_MAX_HEAT || z.heat_w < 0 || z.heat_w > MYDET_ZONE_MAX_HEAT) return false;
    for (int p = 0; p < z.n_polygons; ++p) {
        const int n = z.n_vertices[p];
        if (n < 3 || n > MYDET_ZONE_MAX_VERTICES) return false;
        int64_t area2 = 0;
        for (int i = 0; i < n; ++i) {
            const int *u = z.polygon[p][i], *v = z.polygon[p][(i + 1) % n];
            if (!zone_coord_ok(u[0]) || !zone_coord_ok(u[1])) return false;
            area2 += (int64_t)u[0] * v[1] - (int64_t)v[0] * u[1];
        }
        if (area2 == 0) return false;
    }
    for (int l = 0; l < z.n_lines; ++l) {
        const int *q = z.line[l];
        if (!zone_coord_ok(q[0]) || !zone_coord_ok(q[1]) || !zone_coord_ok(q[2]) || !zone_coord_ok(q[3])) return false;
        if (q[0] == q[2] && q[1] == q[3]) return false;
    }
    return true;
}

}  // namespace

extern "C" int64_t mydet_zones_state_words(int max_tracks) {
    if (max_tracks < 1 || max_tracks > MYDET_TRACK_MAX_TRACKS) return 0;
    return ((int64_t)MYDET_ZONES_STATE_HEADER + (int64_t)MYDET_ZONES_SLOT_WORDS * max_tracks + 3) / 4 * 4;
}

extern "C" int mydet_zones_reset(int32_t *state, int S, int max_tracks, void *stream) {
    if (S <= 0 || max_tracks < 1 || !state || ((uintptr_t)state & 15)) return MYDET_E_BADARG;
    if (max_tracks > MYDET_TRACK_MAX_TRACKS) return MYDET_E_UNSUPP;
    hipLaunchKernelGGL(zones_reset_kernel, dim3((unsigned)S), dim3(256), 0, (hipStream_t)stream, state, mydet_zones_state_words(max_tracks));
    return mydet_launch_status();
}

extern "C" int mydet_zones_frames(const float *box, const int64_t *id, const int64_t *cls, const int32_t *missed, const int32_t *count,
                                  int S, int F, int max_tracks, const mydet_zone_set *zs, int32_t *state, int32_t *heat,
                                  int32_t *out_inside, int32_t *out_crossed, int32_t *out_dwell, int32_t *out_occupancy,
                                  int32_t *out_zone_counts, int32_t *out_line_counts, void *stream) {
    if (S <= 0 || F <= 0 || max_tracks < 1) return MYDET_E_BADARG;
    if (!box || !id || !cls || !missed || !count || !zs || !state || !out_inside || !out_crossed) return MYDET_E_BADARG;
    if (!zone_set_ok(*zs)) return MYDET_E_BADARG;
    if (zs->n_polygons > 0 && (!out_dwell || !out_occupancy || !out_zone_counts)) return MYDET_E_BADARG;
    if (zs->n_lines > 0 && !out_line_counts) return MYDET_E_BADARG;
    if (zs->heat_h > 0 && !heat) return MYDET_E_BADARG;
    if (((uintptr_t)state & 15) || ((uintptr_t)box & 3) || ((uintptr_t)id & 7) || ((uintptr_t)cls & 7) || ((uintptr_t)missed & 3) ||
        ((uintptr_t)count & 3) || ((uintptr_t)heat & 3) || ((uintptr_t)out_inside & 3) || ((uintptr_t)out_crossed & 3) ||
        ((uintptr_t)out_dwell & 3) || ((uintptr_t)out_occupancy & 3) || ((uintptr_t)out_zone_counts & 3) || ((uintptr_t)out_line_counts & 3))
        return MYDET_E_BADARG;
    if (max_tracks > MYDET_TRACK_MAX_TRACKS) return MYDET_E_UNSUPP;
    ZoneArgs a;
    a.box = box; a.id = id; a.cls = cls; a.missed = missed; a.count = count; a.F = F; a.MT = max_tracks;
    a.state = state; a.state_words = mydet_zones_state_words(max_tracks);
    a.heat = heat;
    a.oinside = out_inside; a.ocrossed = out_crossed; a.odwell = out_dwell; a.oocc = out_occupancy; a.ozc = out_zone_counts;
    a.olc = out_line_counts;
    a.zs = *zs;
    hipLaunchKernelGGL(zones_kernel, dim3((unsigned)S), dim3((unsigned)((max_tracks + 63) / 64 * 64)), 0, (hipStream_t)stream, a);
    return mydet_launch_status();
}
