// Counting overlay: zone fills and outlines, directed lines with their ticks, counter labels and track trails painted IN PLACE
// into uint8 RGB frames or the planes of the 8-bit 4:2:0 layouts, one launch per batch, and the launch that keeps the trails
// (include/mydet.h: mydet_draw_overlay_rgb_u8, mydet_draw_overlay_yuv420_u8, mydet_trails_frames, where the rules are; DESIGN.md
// section 4 has the reasoning; tests/_overlay_ref.py restates them in Python).  Every decision is an integer comparison.
//
// The painter sits on the pixel-group frame of paint_tile.h.  One workgroup of 256 lanes per tile; the operations are walked in
// paint order in rounds, each round a compaction of the candidates that reach the tile into LDS followed by every lane walking
// the short list for its own pixels:
//   fills     lanes 0..15 test the polygons' bounding boxes; the survivors are one 16-bit mask
//   strokes   lane = candidate: the polygon edges (z * 16 + e), then the lines and ticks; each is tested against the tile by its
//             bounding box and by the distance of the tile's centre from its line; the survivors become OvSeg records
//   trails    lane = track slot, 256 at a time: out_bbox against the tile; then lane = (surviving trail, segment), 8 trails at a
//             time, tested like a stroke
//   labels    lanes 0..31 format the glyph count of their label, place it and test the rectangle; a survivor writes its text
// A tile without a survivor in any round reads and writes no pixel.  The others load their pixels at the first survivor and
// store the pixel groups that some operation hit.  Every barrier is on workgroup-uniform control flow: the round structure
// depends on the kernel arguments, on the frame's trail lengths through counts every lane reads from LDS, and on nothing else.
#include "draw_yuv.h"
#include "paint_tile.h"

namespace {

constexpr int OV_THREADS = PT_THREADS;
constexpr int OV_Z = MYDET_ZONES_MAX, OV_V = MYDET_ZONE_MAX_VERTICES, OV_NAME = MYDET_DRAW_NAME_BYTES;
constexpr int OV_GLYPHS = MYDET_OVERLAY_MAX_GLYPHS, OV_LP = MYDET_TRAIL_MAX_POINTS;
constexpr int OV_TR_PER_ROUND = OV_THREADS / OV_LP;                   // trails whose segments one round tests
static_assert(OV_THREADS == 256 && OV_LP == 32 && OV_Z * OV_V == OV_THREADS, "the candidate numbering of the rounds");

// A stroke that reaches the tile: a, d = b - a, len2 = d.d, lim = r^2 * len2 (include/mydet.h: both fit int64)
struct OvSeg {
    int ax, ay, dx, dy;
    int64_t len2, lim;
    int r2;
    uint32_t col;                            // r | g << 8 | b << 16, or y | u << 8 | v << 16
};

struct OvLabel {
    int lx, ly, lw;                          // left, top, width in pixels (0: not on this tile); its height is ch
    uint32_t col, tcol;
    unsigned char text[OV_GLYPHS];
};

struct OvArgs {
    mydet_overlay o;
    const unsigned char *palette, *atlas;
    int n_palette, ch, cw;
    int H, W;
    PaintPlanes t;
    DrawYuvK k;
};

// the capsule rule on one pixel centre
__device__ __forceinline__ bool ov_stroke_hit(const OvSeg &s, int px, int py) {
    const int vx = px - s.ax, vy = py - s.ay;
    const int64_t u = (int64_t)vx * s.dx + (int64_t)vy * s.dy;
    if (u <= 0) return (int64_t)vx * vx + (int64_t)vy * vy <= (int64_t)s.r2;
    if (u >= s.len2) {
        const int wx = vx - s.dx, wy = vy - s.dy;
        return (int64_t)wx * wx + (int64_t)wy * wy <= (int64_t)s.r2;
    }
    const int64_t c = (int64_t)s.dx * vy - (int64_t)s.dy * vx;
    if (c >= 2147483648ll || c <= -2147483648ll) return false;       // c^2 >= 2^62 > lim
    return c * c <= s.lim;
}

// Can the stroke a -> b of radius r (fixed point) reach a pixel centre of the tile?  xlo .. yhi: the first and last centres.
// Conservative: the bounding box, then the distance of the tile's centre from the line through a and b in float32 with a
// margin far above its rounding (the test only skips work; the pixels are decided by ov_stroke_hit).
__device__ __forceinline__ bool ov_stroke_reaches(int ax, int ay, int bx, int by, int r, int xlo, int ylo, int xhi, int yhi) {
    if (max(ax, bx) + r < xlo || min(ax, bx) - r > xhi || max(ay, by) + r < ylo || min(ay, by) - r > yhi) return false;
    const float dx = (float)(bx - ax), dy = (float)(by - ay);
    const float len2 = dx * dx + dy * dy;
    if (len2 == 0.0f) return true;
    const float mx = 0.5f * ((float)xlo + (float)xhi) - (float)ax, my = 0.5f * ((float)ylo + (float)yhi) - (float)ay;
    const float hx = 0.5f * (float)(xhi - xlo), hy = 0.5f * (float)(yhi - ylo);
    const float c = dx * my - dy * mx;
    const float reach = ((float)r + 32.0f) * sqrtf(len2) + fabsf(dx) * hy + fabsf(dy) * hx;    // the support of the tile along the normal
    return fabsf(c) <= reach * 1.001f;
}

__device__ __forceinline__ OvSeg ov_seg(int ax, int ay, int bx, int by, int r, uint32_t col) {
    OvSeg s;
    s.ax = ax; s.ay = ay; s.dx = bx - ax; s.dy = by - ay;
    s.len2 = (int64_t)s.dx * s.dx + (int64_t)s.dy * s.dy;
    s.r2 = r * r;
    s.lim = (int64_t)s.r2 * s.len2;
    s.col = col;
    return s;
}

// even-odd, half-open: the rule text of mydet_zones_frames on the raw vertices
__device__ __forceinline__ bool ov_inside(const mydet_overlay_geometry *g, int z, int n, int px, int py) {
    bool in = false;
    for (int e = 0; e < n; ++e) {
        const int e1 = e + 1 == n ? 0 : e + 1;
        const int ax = g->polygon[z][e][0], ay = g->polygon[z][e][1], bx = g->polygon[z][e1][0], by = g->polygon[z][e1][1];
        if ((ay > py) != (by > py)) {
            const int d = by - ay;
            const int64_t lhs = (int64_t)(px - ax) * d, rhs = (int64_t)(bx - ax) * (py - ay);
            in ^= d > 0 ? lhs < rhs : lhs > rhs;
        }
    }
    return in;
}

__device__ __forceinline__ uint32_t ov_palette(const OvArgs &p, int64_t key) {
    key %= p.n_palette;
    if (key < 0) key += p.n_palette;
    const unsigned char *e = p.palette + 3 * key;
    return px_pack(e[0], e[1], e[2]);
}

__device__ __forceinline__ uint32_t ov_text_rgb(uint32_t rgb) {
    return 299 * px_chan(rgb, 0) + 587 * px_chan(rgb, 1) + 114 * px_chan(rgb, 2) < 150000 ? 0xffffffu : 0u;
}

__device__ __forceinline__ int ov_shown(int v) { return v < 0 ? 0 : (v > 999999 ? 999999 : v); }

// `lead`, then the decimal of v (0 .. 999999) into t[n...] when WRITE, never past OV_GLYPHS; returns the new n
template <bool WRITE>
__device__ __forceinline__ int ov_put(unsigned char *t, int n, char sep, char lead, int v) {
    if (n < OV_GLYPHS) { if (WRITE) t[n] = (unsigned char)sep; ++n; }
    if (lead && n < OV_GLYPHS) { if (WRITE) t[n] = (unsigned char)lead; ++n; }
    int p = 1;
    while (v / p >= 10) p *= 10;
    for (; p > 0; p /= 10) {
        const int d = v / p;
        v -= d * p;
        if (n < OV_GLYPHS) { if (WRITE) t[n] = (unsigned char)('0' + d); ++n; }
    }
    return n;
}

// The label of zone i (i < OV_Z) or line i - OV_Z in frame o (include/mydet.h has the rule; ops.overlay_label_text is its host
// form): the glyph count; WRITE: the text into t as well
template <bool WRITE>
__device__ int ov_label_text(const OvArgs &p, int64_t o, int i, unsigned char *t) {
    const unsigned char *nm = p.o.geometry->name[i];
    int n = 0;
    for (; n < OV_NAME && nm[n]; ++n)
        if (WRITE) t[n] = nm[n];
    if (i < OV_Z) {
        const int64_t at = o * p.o.n_polygons + i;
        if (p.o.counters & MYDET_OVERLAY_COUNT_OCCUPANCY) n = ov_put<WRITE>(t, n, ' ', 0, ov_shown(p.o.occupancy[at]));
        if (p.o.counters & MYDET_OVERLAY_COUNT_ENTRIES) n = ov_put<WRITE>(t, n, ' ', '+', ov_shown(p.o.zone_counts[at * 4]));
        if (p.o.counters & MYDET_OVERLAY_COUNT_VISITS) n = ov_put<WRITE>(t, n, ' ', '-', ov_shown(p.o.zone_counts[at * 4 + 3]));
    } else {
        const int64_t at = (o * p.o.n_lines + (i - OV_Z)) * 2;
        n = ov_put<WRITE>(t, n, ' ', '+', ov_shown(p.o.line_counts[at]));
        n = ov_put<WRITE>(t, n, ' ', '-', ov_shown(p.o.line_counts[at + 1]));
    }
    return n;
}

// A lane's pixels in registers: RGB px[k]; 4:2:0 Y[r][k] and the chroma samples of its two quads
template <int FMT>
struct OvPixels {
    int Y[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}}, U[2] = {0, 0}, V[2] = {0, 0};
    bool loaded = false, dirty = false;
};
template <>
struct OvPixels<0> {
    uint32_t px[4] = {0, 0, 0, 0};
    bool loaded = false, dirty = false;
};

__device__ __forceinline__ int ov_blend1(int old, int col, int alpha) { return (col * alpha + old * (255 - alpha) + 127) / 255; }

// One operation on the lane's pixels.  code(i, j): 0 = pixel (i, j) is not hit, 1 = hit with colour ca, 2 = with cb (a label's
// text).  alpha 255: opaque.  A chroma sample takes the operation once, with the colour at the first pixel of its quad that is
// hit, in raster order.
template <int FMT, typename Code>
__device__ __forceinline__ void ov_apply(OvPixels<FMT> &s, const PaintGroup &u, int i0, int j0, uint32_t ca, uint32_t cb, int alpha, Code code) {
    if constexpr (FMT == 0) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (k >= u.nc) continue;
            const int c = code(i0, j0 + k);
            if (!c) continue;
            const uint32_t col = c == 2 ? cb : ca;
            s.px[k] = alpha == 255 ? col
                                   : px_pack(ov_blend1(px_chan(s.px[k], 0), px_chan(col, 0), alpha), ov_blend1(px_chan(s.px[k], 1), px_chan(col, 1), alpha),
                                             ov_blend1(px_chan(s.px[k], 2), px_chan(col, 2), alpha));
            s.dirty = true;
        }
    } else {
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            int first = 0;
#pragma unroll
            for (int r = 0; r < 2; ++r)
#pragma unroll
                for (int k = 2 * q; k < 2 * q + 2; ++k) {
                    if (r >= u.nr || k >= u.nc) continue;
                    const int c = code(i0 + r, j0 + k);
                    if (!c) continue;
                    const int cy = px_chan(c == 2 ? cb : ca, 0);
                    s.Y[r][k] = alpha == 255 ? cy : ov_blend1(s.Y[r][k], cy, alpha);
                    if (!first) first = c;
                }
            if (first) {
                const uint32_t col = first == 2 ? cb : ca;
                s.U[q] = alpha == 255 ? px_chan(col, 1) : ov_blend1(s.U[q], px_chan(col, 1), alpha);
                s.V[q] = alpha == 255 ? px_chan(col, 2) : ov_blend1(s.V[q], px_chan(col, 2), alpha);
                s.dirty = true;
            }
        }
    }
}

template <int FMT>
__device__ __forceinline__ void ov_load(OvPixels<FMT> &s, const PaintPlanes &t, const PaintGroup &u) {
    if (s.loaded || !u.nc) return;
    s.loaded = true;
    if constexpr (FMT == 0) {
        uint32_t px[4] = {0, 0, 0, 0};                                   // an array of its own, as in draw.hip: it stays in registers
        paint_load(u, px);
#pragma unroll
        for (int k = 0; k < 4; ++k) s.px[k] = px[k];
    } else {
        paint_load<FMT>(t, u, s.Y, s.U, s.V);
    }
}

// every lane walks the n strokes of the list for its pixels
template <int FMT>
__device__ __forceinline__ void ov_strokes(OvPixels<FMT> &s, const PaintPlanes &t, const PaintGroup &u, int i0, int j0, const OvSeg *segs, int n) {
    if (!n || !u.nc) return;
    ov_load<FMT>(s, t, u);
    for (int e = 0; e < n; ++e) {
        const OvSeg &g = segs[e];
        ov_apply<FMT>(s, u, i0, j0, g.col, g.col, 255, [&](int i, int j) { return ov_stroke_hit(g, 16 * j + 8, 16 * i + 8) ? 1 : 0; });
    }
}

template <int FMT>
__global__ __launch_bounds__(OV_THREADS) void overlay_kernel(const OvArgs p) {
    __shared__ OvSeg segs[OV_THREADS];
    __shared__ OvLabel labels[2 * OV_Z];
    __shared__ int trails[OV_THREADS];                                   // the slots of the trails that reach the tile
    __shared__ int wave_cnt[OV_THREADS / 64];
    __shared__ unsigned s_fill, s_labels;
    constexpr int TW = FMT == 0 ? 64 : 128;
    const int tid = threadIdx.x, b = blockIdx.z;
    const int tx0 = blockIdx.x * TW, ty0 = blockIdx.y * 16;
    const int i0 = FMT == 0 ? ty0 + (tid >> 4) : ty0 + 2 * (tid >> 5);
    const int j0 = FMT == 0 ? tx0 + 4 * (tid & 15) : tx0 + 4 * (tid & 31);
    const PaintGroup u = paint_group<FMT>(p.t, p.H, p.W, b, i0, j0);
    // the centres of the tile's first and last pixel inside the frame, in fixed point
    const int xlo = 16 * tx0 + 8, ylo = 16 * ty0 + 8, xhi = 16 * min(tx0 + TW - 1, p.W - 1) + 8, yhi = 16 * min(ty0 + 15, p.H - 1) + 8;
    const mydet_overlay_geometry *g = p.o.geometry;
    const int nz = (p.o.flags & MYDET_OVERLAY_ZONES) ? p.o.n_polygons : 0, nl = (p.o.flags & MYDET_OVERLAY_LINES) ? p.o.n_lines : 0;
    const int64_t o = b;
    OvPixels<FMT> s;

    if (tid == 0) { s_fill = 0u; s_labels = 0u; }
    __syncthreads();

    // ---- fills
    if (nz > 0) {
        if (tid < nz) {
            const int n = min(g->n_vertices[tid], OV_V);
            int x0 = INT32_MAX, y0 = INT32_MAX, x1 = INT32_MIN, y1 = INT32_MIN;
            for (int e = 0; e < n; ++e) {
                const int x = g->polygon[tid][e][0], y = g->polygon[tid][e][1];
                x0 = min(x0, x); x1 = max(x1, x); y0 = min(y0, y); y1 = max(y1, y);
            }
            const int alpha = p.o.occupancy[o * p.o.n_polygons + tid] == 0 ? p.o.zone_alpha : p.o.occupied_alpha;
            if (n >= 3 && alpha > 0 && !(x1 < xlo || x0 > xhi || y1 < ylo || y0 > yhi)) atomicOr(&s_fill, 1u << tid);
        }
        __syncthreads();
        const unsigned fill = s_fill;
        if (fill && u.nc) {
            ov_load<FMT>(s, p.t, u);
            for (int z = 0; z < nz; ++z) {
                if (!((fill >> z) & 1u)) continue;
                const int n = min(g->n_vertices[z], OV_V);
                const int alpha = p.o.occupancy[o * p.o.n_polygons + z] == 0 ? p.o.zone_alpha : p.o.occupied_alpha;
                const uint32_t rgb = ov_palette(p, z), col = FMT ? draw_yuv_of(p.k, rgb) : rgb;
                ov_apply<FMT>(s, u, i0, j0, col, col, alpha, [&](int i, int j) { return ov_inside(g, z, n, 16 * j + 8, 16 * i + 8) ? 1 : 0; });
            }
        }
    }

    // ---- zone outlines: candidate c = z * 16 + e
    if (nz > 0) {
        const int z = tid >> 4, e = tid & 15, r = 8 * p.o.thickness;
        const int n = z < nz ? min(g->n_vertices[z], OV_V) : 0;
        int ax = 0, ay = 0, bx = 0, by = 0;
        bool hit = false;
        if (e < n) {
            const int e1 = e + 1 == n ? 0 : e + 1;
            ax = g->polygon[z][e][0]; ay = g->polygon[z][e][1]; bx = g->polygon[z][e1][0]; by = g->polygon[z][e1][1];
            hit = ov_stroke_reaches(ax, ay, bx, by, r, xlo, ylo, xhi, yhi);
        }
        const int cnt = paint_compact(hit, wave_cnt, [&](int slot) {
            const uint32_t rgb = ov_palette(p, z);
            segs[slot] = ov_seg(ax, ay, bx, by, r, FMT ? draw_yuv_of(p.k, rgb) : rgb);
        });
        ov_strokes<FMT>(s, p.t, u, i0, j0, segs, cnt);
        __syncthreads();                                                 // the list is rewritten by the next round
    }

    // ---- lines, each followed by its tick: candidate c = 2 l + (0 line | 1 tick)
    if (nl > 0) {
        const int l = tid >> 1, r = 8 * p.o.thickness;
        int ax = 0, ay = 0, bx = 0, by = 0;
        bool hit = false;
        if (l < nl) {
            const int *q = (tid & 1) ? g->tick[l] : g->line[l];
            ax = q[0]; ay = q[1]; bx = q[2]; by = q[3];
            hit = ov_stroke_reaches(ax, ay, bx, by, r, xlo, ylo, xhi, yhi);
        }
        const int cnt = paint_compact(hit, wave_cnt, [&](int slot) {
            const uint32_t rgb = ov_palette(p, l);
            segs[slot] = ov_seg(ax, ay, bx, by, r, FMT ? draw_yuv_of(p.k, rgb) : rgb);
        });
        ov_strokes<FMT>(s, p.t, u, i0, j0, segs, cnt);
        __syncthreads();
    }

    // ---- trails, by slot
    if (p.o.flags & MYDET_OVERLAY_TRAILS) {
        const int MT = p.o.max_tracks, L = p.o.max_points, r = 8 * p.o.trail_thickness;
        for (int base = 0; base < MT; base += OV_THREADS) {
            const int t = base + tid;
            bool hit = false;
            if (t < MT) {
                const int64_t at = o * MT + t;
                const int ms = p.o.missed[at];
                if (p.o.trail_len[at] >= 2 && (ms == 0 || (p.o.coasting && ms > 0))) {
                    const int32_t *bb = p.o.trail_bbox + at * 4;
                    hit = !(bb[2] + r < xlo || bb[0] - r > xhi || bb[3] + r < ylo || bb[1] - r > yhi);
                }
            }
            const int n_tr = paint_compact(hit, wave_cnt, [&](int slot) { trails[slot] = t; });
            for (int g0 = 0; g0 < n_tr; g0 += OV_TR_PER_ROUND) {         // n_tr is the same for every lane
                const int j = g0 + (tid >> 5), kk = tid & 31;
                int ax = 0, ay = 0, bx = 0, by = 0;
                int64_t at = 0;
                bool seg_hit = false;
                if (j < n_tr) {
                    at = o * MT + trails[j];
                    const int len = min(p.o.trail_len[at], L);
                    if (kk + 1 < len) {
                        const int32_t *pt = p.o.trail_points + (at * L + kk) * 2;
                        ax = pt[0]; ay = pt[1]; bx = pt[2]; by = pt[3];
                        seg_hit = ov_stroke_reaches(ax, ay, bx, by, r, xlo, ylo, xhi, yhi);
                    }
                }
                const int cnt = paint_compact(seg_hit, wave_cnt, [&](int slot) {
                    const uint32_t rgb = ov_palette(p, p.o.id[at]);
                    segs[slot] = ov_seg(ax, ay, bx, by, r, FMT ? draw_yuv_of(p.k, rgb) : rgb);
                });
                ov_strokes<FMT>(s, p.t, u, i0, j0, segs, cnt);
                __syncthreads();
            }
            __syncthreads();                                             // `trails` is rewritten by the next 256 slots
        }
    }

    // ---- labels: zone z at lane z, line l at lane 16 + l
    if (p.o.counters && (nz > 0 || nl > 0)) {
        if (tid < 2 * OV_Z) {
            OvLabel &lb = labels[tid];
            lb.lw = 0;
            const bool have = tid < OV_Z ? tid < nz : tid - OV_Z < nl;
            if (have) {
                const int lw = ov_label_text<false>(p, o, tid, nullptr) * p.cw;
                if (lw > 0) {
                    const int mx = p.W - lw > 0 ? p.W - lw : 0, my = p.H - p.ch > 0 ? p.H - p.ch : 0;
                    const int lx = px_clamp(g->anchor[tid][0] >> 4, 0, mx), ly = px_clamp((g->anchor[tid][1] >> 4) - p.ch, 0, my);
                    if (lx < tx0 + TW && lx + lw > tx0 && ly < ty0 + 16 && ly + p.ch > ty0) {
                        const uint32_t rgb = ov_palette(p, tid < OV_Z ? tid : tid - OV_Z), trgb = ov_text_rgb(rgb);
                        lb.lx = lx; lb.ly = ly; lb.lw = lw;
                        lb.col = FMT ? draw_yuv_of(p.k, rgb) : rgb;
                        lb.tcol = FMT ? draw_yuv_of(p.k, trgb) : trgb;
                        ov_label_text<true>(p, o, tid, lb.text);
                        atomicOr(&s_labels, 1u << tid);
                    }
                }
            }
        }
        __syncthreads();
        const unsigned lab = s_labels;
        if (lab && u.nc) {
            ov_load<FMT>(s, p.t, u);
            for (int e = 0; e < 2 * OV_Z; ++e) {
                if (!((lab >> e) & 1u)) continue;
                const OvLabel &lb = labels[e];
                ov_apply<FMT>(s, u, i0, j0, lb.col, lb.tcol, 255, [&](int i, int j) {
                    const unsigned lr = (unsigned)(i - lb.ly), lc = (unsigned)(j - lb.lx);
                    if (lc >= (unsigned)lb.lw || lr >= (unsigned)p.ch) return 0;
                    const unsigned gi = lc / (unsigned)p.cw, q = lc - gi * (unsigned)p.cw;
                    unsigned code = lb.text[gi];
                    if (code < 32u || code > 127u) code = '?';
                    return p.atlas[((size_t)(code - 32u) * p.ch + lr) * p.cw + q] ? 2 : 1;
                });
            }
        }
    }

    if (s.dirty) {
        if constexpr (FMT == 0) paint_store(u, s.px, paint_inside(u));
        else paint_store<FMT>(p.t, u, s.Y, s.U, s.V, paint_inside(u), paint_quads(paint_inside(u)));
    }
}

// The checks both entry points share
int overlay_check(const mydet_overlay *o, const mydet_draw_style *s, int B, int H, int W) {
    if (!o || !s || B <= 0 || H <= 0 || W <= 0 || H > MYDET_ZONE_MAX_FRAME || W > MYDET_ZONE_MAX_FRAME) return MYDET_E_BADARG;
    const int all = MYDET_OVERLAY_ZONES | MYDET_OVERLAY_LINES | MYDET_OVERLAY_TRAILS;
    const int parts = MYDET_OVERLAY_COUNT_OCCUPANCY | MYDET_OVERLAY_COUNT_ENTRIES | MYDET_OVERLAY_COUNT_VISITS;
    if (!o->flags || (o->flags & ~all) || (o->counters & ~parts)) return MYDET_E_BADARG;
    if (!s->palette || s->n_palette < 1) return MYDET_E_BADARG;
    if (o->S < 1 || o->F < 1 || (int64_t)o->S * o->F != (int64_t)B) return MYDET_E_BADARG;
    if (o->zone_alpha < 0 || o->zone_alpha > 255 || o->occupied_alpha < 0 || o->occupied_alpha > 255) return MYDET_E_BADARG;
    if (o->thickness < 1 || o->thickness > MYDET_DRAW_MAX_THICKNESS || o->trail_thickness < 1 || o->trail_thickness > MYDET_DRAW_MAX_THICKNESS)
        return MYDET_E_BADARG;
    if (o->n_polygons < 0 || o->n_polygons > MYDET_ZONES_MAX || o->n_lines < 0 || o->n_lines > MYDET_ZONES_MAX) return MYDET_E_BADARG;
    if (o->coasting != 0 && o->coasting != 1) return MYDET_E_BADARG;
    const bool zones = (o->flags & MYDET_OVERLAY_ZONES) && o->n_polygons > 0, lines = (o->flags & MYDET_OVERLAY_LINES) && o->n_lines > 0;
    if ((o->flags & (MYDET_OVERLAY_ZONES | MYDET_OVERLAY_LINES)) && !o->geometry) return MYDET_E_BADARG;
    if (zones && !o->occupancy) return MYDET_E_BADARG;
    if (o->counters && (zones || lines)) {
        if ((zones && !o->zone_counts) || (lines && !o->line_counts)) return MYDET_E_BADARG;
        if (!s->atlas || s->ch < 8 || s->ch > 64 || s->cw < 1 || s->cw > 64) return MYDET_E_BADARG;
    }
    if (o->flags & MYDET_OVERLAY_TRAILS) {
        if (o->max_tracks < 1 || o->max_points < 2 || o->max_points > MYDET_TRAIL_MAX_POINTS) return MYDET_E_BADARG;
        if (!o->trail_points || !o->trail_len || !o->trail_bbox || !o->id || !o->missed) return MYDET_E_BADARG;
        if (((uintptr_t)o->trail_points & 3) || ((uintptr_t)o->trail_len & 3) || ((uintptr_t)o->trail_bbox & 3) || ((uintptr_t)o->id & 7) ||
            ((uintptr_t)o->missed & 3))
            return MYDET_E_BADARG;
    }
    if (((uintptr_t)o->geometry & 3) || ((uintptr_t)o->occupancy & 3) || ((uintptr_t)o->zone_counts & 3) || ((uintptr_t)o->line_counts & 3))
        return MYDET_E_BADARG;
    if ((o->flags & MYDET_OVERLAY_TRAILS) && o->max_tracks > MYDET_TRACK_MAX_TRACKS) return MYDET_E_UNSUPP;
    return 0;
}

template <typename Kernel>
int overlay_launch(Kernel kernel, OvArgs &p, int TW, int B, int H, int W, const mydet_overlay *o, const mydet_draw_style *s, void *stream) {
    const int gy = (H + 15) / 16;
    if (B > 65535 || gy > 65535) return MYDET_E_UNSUPP;
    p.o = *o; p.palette = s->palette; p.atlas = s->atlas; p.n_palette = s->n_palette; p.ch = s->ch; p.cw = s->cw; p.H = H; p.W = W;
    const dim3 grid((unsigned)((W + TW - 1) / TW), (unsigned)gy, (unsigned)B);
    hipLaunchKernelGGL(kernel, grid, dim3(OV_THREADS), 0, (hipStream_t)stream, p);
    return mydet_launch_status();
}

// --------------------------------------------------------------------------------------------------------------- trails
struct TrailArgs {
    const float *box;
    const int64_t *id, *cls;
    const int32_t *missed, *count;
    int F, MT;
    int32_t *state;
    int64_t state_words;                     // per stream
    int32_t *opoints, *olen, *obbox;
    mydet_trail_set ts;
};

__device__ __forceinline__ bool trail_finite(float v) { return v - v == 0.0f; }
__device__ __forceinline__ int trail_q(float v) { return (int)floorf(fminf(fmaxf(v * 16.0f, -1048576.0f), 1048576.0f)); }

// No barrier and no LDS: a slot's ring lives in the state, which its own thread alone reads and writes
__global__ __launch_bounds__(MYDET_TRACK_MAX_TRACKS) void trails_kernel(const TrailArgs a) {
    const int tid = threadIdx.x, s = blockIdx.x, MT = a.MT, F = a.F, L = a.ts.max_points, ncls = a.ts.n_classes;
    if (tid >= MT) return;
    const bool bottom = a.ts.anchor == MYDET_ZONE_ANCHOR_BOTTOM;
    int32_t *st = a.state + (int64_t)s * a.state_words;
    int64_t *g_id = reinterpret_cast<int64_t *>(st);
    int32_t *g_fill = st + 2 * MT, *g_head = g_fill + MT, *ring = g_head + MT + (int64_t)tid * L * 2;
    int64_t sid = g_id[tid];
    int fill = px_clamp(g_fill[tid], 0, L), head = px_clamp(g_head[tid], 0, L - 1);    // a state of another L cannot index out of the ring
    for (int f = 0; f < F; ++f) {
        const int64_t o = (int64_t)s * F + f, at = o * MT + tid;
        const int64_t id = a.id[at];
        if (a.count[o] >= 0) {
            if (sid != 0 && sid != id) {                                 // 2. clear
                sid = 0; fill = 0; head = 0;
                for (int k = 0; k < 2 * L; ++k) ring[k] = 0;
            }
            if (id != 0 && a.missed[at] == 0) {                          // 3. push
                bool obs = true;
                if (ncls > 0) {
                    const int64_t c = a.cls[at];
                    obs = false;
                    for (int i = 0; i < ncls; ++i) obs = obs || c == (int64_t)a.ts.classes[i];
                }
                float fx = 0.0f, fy = 0.0f;
                if (obs) {
                    const float *bx = a.box + at * 5;
                    fx = bx[0];
                    fy = bottom ? bx[1] + bx[3] / 2.0f : bx[1];
                    obs = trail_finite(fx) && trail_finite(fy);
                }
                if (obs) {
                    if (sid == 0) sid = id;
                    ring[2 * head] = trail_q(fx); ring[2 * head + 1] = trail_q(fy);
                    head = head + 1 == L ? 0 : head + 1;
                    fill = min(fill + 1, L);
                }
            }
        }
        // 4. outputs
        int32_t *op = a.opoints + at * L * 2;
        int x0 = 0, y0 = 0, x1 = 0, y1 = 0, idx = head;
        for (int k = 0; k < L; ++k) {
            idx = idx == 0 ? L - 1 : idx - 1;
            int x = 0, y = 0;
            if (k < fill) {
                x = ring[2 * idx]; y = ring[2 * idx + 1];
                if (k == 0) { x0 = x1 = x; y0 = y1 = y; }
                x0 = min(x0, x); x1 = max(x1, x); y0 = min(y0, y); y1 = max(y1, y);
            }
            op[2 * k] = x; op[2 * k + 1] = y;
        }
        a.olen[at] = sid == id ? fill : 0;
        int32_t *ob = a.obbox + at * 4;
        ob[0] = x0; ob[1] = y0; ob[2] = x1; ob[3] = y1;
    }
    g_id[tid] = sid; g_fill[tid] = fill; g_head[tid] = head;
}

__global__ __launch_bounds__(256) void trails_reset_kernel(int32_t *state, int64_t words) {
    int32_t *st = state + (int64_t)blockIdx.x * words;
    for (int64_t i = threadIdx.x; i < words; i += 256) st[i] = 0;
}

inline bool trail_points_ok(int max_points) { return max_points >= 2 && max_points <= MYDET_TRAIL_MAX_POINTS; }

}  // namespace

extern "C" int mydet_draw_overlay_rgb_u8(unsigned char *dst, int B, int H, int W, int64_t dst_img_bytes, int64_t dst_row_bytes,
                                         const mydet_overlay *overlay, const mydet_draw_style *style, void *stream) {
    OvArgs p = {};
    int code = overlay_check(overlay, style, B, H, W);
    if (!code) code = paint_planes_rgb(p.t, dst, dst_img_bytes, dst_row_bytes, W);
    if (code) return code;
    return overlay_launch(overlay_kernel<0>, p, 64, B, H, W, overlay, style, stream);
}

extern "C" int mydet_draw_overlay_yuv420_u8(const mydet_yuv420_src *planes, int B, int H, int W, const mydet_overlay *overlay,
                                            const mydet_draw_style *style, void *stream) {
    OvArgs p = {};
    int code = overlay_check(overlay, style, B, H, W);
    if (!code) code = paint_planes_yuv420(p.t, planes, W);
    if (code) return code;
    p.k = DRAW_YUV[planes->matrix][planes->full_range];
    const bool planar = planes->layout == MYDET_YUV420_I420;
    return overlay_launch(planar ? overlay_kernel<2> : overlay_kernel<1>, p, 128, B, H, W, overlay, style, stream);
}

extern "C" int64_t mydet_trails_state_words(int max_tracks, int max_points) {
    if (max_tracks < 1 || max_tracks > MYDET_TRACK_MAX_TRACKS || !trail_points_ok(max_points)) return 0;
    return ((int64_t)max_tracks * (4 + 2 * max_points) + 3) / 4 * 4;
}

extern "C" int mydet_trails_reset(int32_t *state, int S, int max_tracks, int max_points, void *stream) {
    if (S <= 0 || max_tracks < 1 || !trail_points_ok(max_points) || !state || ((uintptr_t)state & 15)) return MYDET_E_BADARG;
    if (max_tracks > MYDET_TRACK_MAX_TRACKS) return MYDET_E_UNSUPP;
    hipLaunchKernelGGL(trails_reset_kernel, dim3((unsigned)S), dim3(256), 0, (hipStream_t)stream, state,
                       mydet_trails_state_words(max_tracks, max_points));
    return mydet_launch_status();
}

extern "C" int mydet_trails_frames(const float *box, const int64_t *id, const int64_t *cls, const int32_t *missed, const int32_t *count,
                                   int S, int F, int max_tracks, const mydet_trail_set *ts, int32_t *state, int32_t *out_points,
                                   int32_t *out_len, int32_t *out_bbox, void *stream) {
    if (S <= 0 || F <= 0 || max_tracks < 1) return MYDET_E_BADARG;
    if (!box || !id || !cls || !missed || !count || !ts || !state || !out_points || !out_len || !out_bbox) return MYDET_E_BADARG;
    if (!trail_points_ok(ts->max_points) || ts->n_classes < 0 || ts->n_classes > MYDET_ZONE_MAX_CLASSES) return MYDET_E_BADARG;
    if (ts->anchor != MYDET_ZONE_ANCHOR_CENTER && ts->anchor != MYDET_ZONE_ANCHOR_BOTTOM) return MYDET_E_BADARG;
    if (((uintptr_t)state & 15) || ((uintptr_t)box & 3) || ((uintptr_t)id & 7) || ((uintptr_t)cls & 7) || ((uintptr_t)missed & 3) ||
        ((uintptr_t)count & 3) || ((uintptr_t)out_points & 3) || ((uintptr_t)out_len & 3) || ((uintptr_t)out_bbox & 3))
        return MYDET_E_BADARG;
    if (max_tracks > MYDET_TRACK_MAX_TRACKS) return MYDET_E_UNSUPP;
    TrailArgs a;
    a.box = box; a.id = id; a.cls = cls; a.missed = missed; a.count = count; a.F = F; a.MT = max_tracks;
    a.state = state; a.state_words = mydet_trails_state_words(max_tracks, ts->max_points);
    a.opoints = out_points; a.olen = out_len; a.obbox = out_bbox;
    a.ts = *ts;
    hipLaunchKernelGGL(trails_kernel, dim3((unsigned)S), dim3((unsigned)((max_tracks + 63) / 64 * 64)), 0, (hipStream_t)stream, a);
    return mydet_launch_status();
}
