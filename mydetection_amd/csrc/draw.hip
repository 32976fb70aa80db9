// Overlay renderer: outlines of axis-aligned and rotated boxes, translucent fills and text labels painted IN PLACE into uint8
// RGB frames or into the planes of the 8-bit 4:2:0 layouts, one launch per batch (include/mydet.h: mydet_draw_boxes_rgb_u8,
// mydet_draw_boxes_yuv420_u8, where the raster rules are; DESIGN.md has them too).  Built with -ffp-contract=off: the
// thresholds of the rules are float32 expressions that must not be fused.
//
// Tiles and a lane's pixel group are paint_tile.h's.  The frame's rows are walked in paint order (count - 1 down to 0) in chunks
// of 256: every lane tests one row against the tile -- the bounding box of the outer rectangle, one pixel wider, less (without a
// fill) the tiles that lie inside the outline's hole, united with the label rectangle -- and the hits are compacted in paint
// order into LDS (geometry, colours, label text: 84 bytes each, 21 KiB).  A tile without a hit in any chunk reads and writes no
// pixel.  The others load their pixels once, walk the short list per pixel and store the pixel groups that changed.
#include "draw_yuv.h"
#include "paint_tile.h"

namespace {

constexpr int DR_THREADS = PT_THREADS;
constexpr int DR_TEXT = 36;                  // bytes of label text kept per hit (MYDET_DRAW_MAX_GLYPHS = 33 used)
constexpr int DR_GLYPHS = 33;
constexpr int DR_NAME = 16;                  // MYDET_DRAW_NAME_BYTES

struct DrawHit {
    float cx, cy, hw, hh, c, s;              // centre, half sizes, cos, sin
    uint32_t col, tcol;                      // box colour and text colour: r | g << 8 | b << 16, or y | u << 8 | v << 16
    int lx, ly, lw, pad;                     // label rectangle: left, top, width in pixels (0 = no label); its height is ch
    unsigned char text[DR_TEXT];
};

struct DrawArgs {
    mydet_draw_list l;
    mydet_draw_style s;
    int H, W;
    PaintPlanes t;
    DrawYuvK k;
};

// (colour * alpha + old * (255 - alpha) + 127) / 255 on one 8-bit value
__device__ __forceinline__ int draw_blend1(int old, int col, int alpha) { return (col * alpha + old * (255 - alpha) + 127) / 255; }
__device__ __forceinline__ uint32_t draw_blend(uint32_t old, uint32_t col, int alpha) {
    return px_pack(draw_blend1(px_chan(old, 0), px_chan(col, 0), alpha), draw_blend1(px_chan(old, 1), px_chan(col, 1), alpha),
                   draw_blend1(px_chan(old, 2), px_chan(col, 2), alpha));
}

// decimal digits of v into t[n...], never past t[cap - 1]; returns the new n
__device__ int draw_put_dec(unsigned char *t, int n, int cap, uint64_t v) {
    uint64_t p = 1;
    while (v / p >= 10) p *= 10;
    for (; p > 0; p /= 10) {
        const uint64_t d = v / p;
        v -= d * p;
        if (n < cap) t[n++] = (unsigned char)('0' + (int)d);
    }
    return n;
}

__device__ int draw_dec_len(uint64_t v) {
    int n = 1;
    for (uint64_t p = 10; v >= p; p *= 10) {
        ++n;
        if (p > 1000000000000000000ull) break;                           // 20 digits: p * 10 would wrap
    }
    return n;
}

// Glyph count of the label of row `r` of frame `b`: what draw_label_text below writes, without writing it
__device__ int draw_label_len(const mydet_draw_list &l, const mydet_draw_style &s, int b, int r) {
    int n = 0;
    if ((s.label_flags & MYDET_DRAW_LABEL_CLASS) && l.cls) {
        const int64_t c = l.cls[(int64_t)b * l.cls_frame_stride + (int64_t)r * l.cls_row_stride];
        if (s.names && c >= 0 && c < s.n_names) {
            const unsigned char *nm = s.names + c * DR_NAME;
            while (n < DR_NAME && nm[n]) ++n;
        } else {
            n = (c < 0) + draw_dec_len(c < 0 ? (uint64_t)0 - (uint64_t)c : (uint64_t)c);
            if (n > DR_NAME) n = DR_NAME;
        }
    }
    if ((s.label_flags & MYDET_DRAW_LABEL_SCORE) && l.score) n += n ? 5 : 4;
    if ((s.label_flags & MYDET_DRAW_LABEL_ID) && l.id) {
        const int64_t m = 10000000000ll;
        int64_t v = l.id[(int64_t)b * l.id_frame_stride + (int64_t)r * l.id_row_stride] % m;
        if (v < 0) v += m;
        n += (n ? 2 : 1) + draw_dec_len((uint64_t)v);
    }
    return n;
}

// The label text of row `r` of frame `b` (include/mydet.h has the rule; ops.draw_label_text is its host form); returns the glyph count
__device__ int draw_label_text(const mydet_draw_list &l, const mydet_draw_style &s, int b, int r, unsigned char *t) {
    int n = 0;
    if ((s.label_flags & MYDET_DRAW_LABEL_CLASS) && l.cls) {
        const int64_t c = l.cls[(int64_t)b * l.cls_frame_stride + (int64_t)r * l.cls_row_stride];
        if (s.names && c >= 0 && c < s.n_names) {
            const unsigned char *nm = s.names + c * DR_NAME;
            for (int k = 0; k < DR_NAME && nm[k]; ++k) t[n++] = nm[k];
        } else {
            if (c < 0) t[n++] = '-';
            n = draw_put_dec(t, n, DR_NAME, c < 0 ? (uint64_t)0 - (uint64_t)c : (uint64_t)c);
        }
    }
    if ((s.label_flags & MYDET_DRAW_LABEL_SCORE) && l.score) {
        const float sc = l.score[(int64_t)b * l.score_frame_stride + (int64_t)r * l.score_row_stride];
        int v = 0;
        if (sc > 0.0f) {                                                  // NaN and negative scores: 0
            const float f = sc * 100.0f + 0.5f;
            v = f >= 100.0f ? 100 : (int)floorf(f);
        }
        if (n) t[n++] = ' ';
        t[n++] = (unsigned char)('0' + v / 100);
        t[n++] = '.';
        t[n++] = (unsigned char)('0' + (v / 10) % 10);
        t[n++] = (unsigned char)('0' + v % 10);
    }
    if ((s.label_flags & MYDET_DRAW_LABEL_ID) && l.id) {
        const int64_t m = 10000000000ll;
        int64_t v = l.id[(int64_t)b * l.id_frame_stride + (int64_t)r * l.id_row_stride] % m;
        if (v < 0) v += m;
        if (n) t[n++] = ' ';
        t[n++] = '#';
        n = draw_put_dec(t, n, DR_GLYPHS, (uint64_t)v);
    }
    return n;
}

// Rows hi, hi - 1, ... (one per lane, down to row 0) of frame b against the tile [tx0, tx0 + TW) x [ty0, ty0 + TH): the hits, in
// that order, into `hits`; returns their number.  Every lane of the workgroup calls it (two barriers inside).
template <bool YUV>
__device__ int draw_collect(const DrawArgs &p, int b, int hi, int tx0, int ty0, int TW, int TH, DrawHit *hits, int *wave_cnt) {
    const int r = hi - (int)threadIdx.x;
    const mydet_draw_list &l = p.l;
    const float ht = (float)p.s.thickness * 0.5f;
    bool hit = false;
    PaintRow g = {0, 0, 0, 0, 1.0f, 0.0f};
    int lx = 0, ly = 0, lw = 0;
    bool ok = false;
    if (r >= 0) {                                                         // the row reader of paint_tile.h, kept here: see paint_row
        const float *bx = l.box + (int64_t)b * l.box_frame_stride + (int64_t)r * l.box_row_stride;
        g.cx = bx[0]; g.cy = bx[1]; g.w = bx[2]; g.h = bx[3];
        const float ang = l.angle ? l.angle[(int64_t)b * l.angle_frame_stride + (int64_t)r * l.angle_row_stride] : 0.0f;
        ok = isfinite(g.cx) && isfinite(g.cy) && isfinite(g.w) && isfinite(g.h) && isfinite(ang) && g.w > 0.0f && g.h > 0.0f;
        if (ok) box_rotation<false>(ang, g.c, g.s);
    }
    if (ok) {
        const float cx = g.cx, cy = g.cy, w = g.w, h = g.h, c = g.c, s = g.s;
        const float ow = w * 0.5f + ht, oh = h * 0.5f + ht;
        float ex, ey;
        paint_extents(c, s, ow, oh, ex, ey);
        hit = paint_reaches(cx, cy, ex, ey, (float)tx0, (float)ty0, (float)(tx0 + TW), (float)(ty0 + TH));
        if (hit && p.s.fill_alpha == 0) {                                 // no fill: a tile inside the outline's hole is not hit
            const float iw = w * 0.5f - ht - 1.0f, ih = h * 0.5f - ht - 1.0f;        // the hole, one pixel smaller
            bool inside = true;
#pragma unroll
            for (int k = 0; k < 4; ++k) {                                 // the hole is convex: the four corners decide
                const float dx = (float)(tx0 + (k & 1) * TW) - cx, dy = (float)(ty0 + (k >> 1) * TH) - cy;
                inside = inside && fabsf(dx * c + dy * s) < iw && fabsf(dy * c - dx * s) < ih;
            }
            hit = !inside;
        }
        if (p.s.label_flags) {                                            // the label rectangle needs the glyph count alone
            const int n = draw_label_len(l, p.s, b, r);
            lw = n * p.s.cw;
            if (lw > 0) {
                const float fx = floorf(cx - w * 0.5f - ht), fy = floorf(cy - h * 0.5f - ht) - (float)p.s.ch;
                const int mx = p.W - lw > 0 ? p.W - lw : 0, my = p.H - p.s.ch > 0 ? p.H - p.s.ch : 0;
                lx = (int)fminf(fmaxf(fx, 0.0f), (float)mx);
                ly = (int)fminf(fmaxf(fy, 0.0f), (float)my);
                if (lx < tx0 + TW && lx + lw > tx0 && ly < ty0 + TH && ly + p.s.ch > ty0) hit = true;
            }
        }
    }
    return paint_compact(hit, wave_cnt, [&](int slot) {
        DrawHit &o = hits[slot];
        o.cx = g.cx; o.cy = g.cy; o.hw = g.w * 0.5f; o.hh = g.h * 0.5f; o.c = g.c; o.s = g.s;
        uint32_t rgb = px_pack(p.s.color[0], p.s.color[1], p.s.color[2]);
        if (p.s.color_mode != MYDET_DRAW_COLOR_FIXED) {
            const int64_t *keys = p.s.color_mode == MYDET_DRAW_COLOR_CLASS ? l.cls : l.id;
            const int64_t fs = p.s.color_mode == MYDET_DRAW_COLOR_CLASS ? l.cls_frame_stride : l.id_frame_stride;
            const int64_t rs = p.s.color_mode == MYDET_DRAW_COLOR_CLASS ? l.cls_row_stride : l.id_row_stride;
            int64_t key = keys ? keys[(int64_t)b * fs + (int64_t)r * rs] % p.s.n_palette : 0;
            if (key < 0) key += p.s.n_palette;
            const unsigned char *e = p.s.palette + 3 * key;
            rgb = px_pack(e[0], e[1], e[2]);
        }
        const bool white = 299 * px_chan(rgb, 0) + 587 * px_chan(rgb, 1) + 114 * px_chan(rgb, 2) < 150000;
        const uint32_t trgb = white ? 0xffffffu : 0u;
        o.col = YUV ? draw_yuv_of(p.k, rgb) : rgb;
        o.tcol = YUV ? draw_yuv_of(p.k, trgb) : trgb;
        o.lx = lx; o.ly = ly; o.lw = lw; o.pad = 0;
        if (lw > 0) draw_label_text(l, p.s, b, r, o.text);
    });
}

// What the hit paints at pixel (i, j): bit 0 fill, bit 1 outline, bit 2 label, bit 3 label text (with bit 2)
__device__ __forceinline__ int draw_ops(const DrawHit &h, const mydet_draw_style &st, float ht, int i, int j) {
    const float dx = ((float)j + 0.5f) - h.cx, dy = ((float)i + 0.5f) - h.cy;
    const float a = fabsf(dx * h.c + dy * h.s), bb = fabsf(dy * h.c - dx * h.s);
    int ops = 0;
    if (a <= h.hw && bb <= h.hh) ops |= 1;
    if (a <= h.hw + ht && bb <= h.hh + ht && !(a < h.hw - ht && bb < h.hh - ht)) ops |= 2;
    const unsigned lr = (unsigned)(i - h.ly), lc = (unsigned)(j - h.lx);
    if (lc < (unsigned)h.lw && lr < (unsigned)st.ch) {
        const unsigned g = lc / (unsigned)st.cw, q = lc - g * (unsigned)st.cw;
        unsigned code = h.text[g];
        if (code < 32u || code > 127u) code = '?';
        ops |= st.atlas[((size_t)(code - 32u) * st.ch + lr) * st.cw + q] ? 12 : 4;
    }
    return ops;
}

__global__ __launch_bounds__(DR_THREADS) void draw_rgb_kernel(const DrawArgs p) {
    __shared__ DrawHit hits[DR_THREADS];
    __shared__ int wave_cnt[DR_THREADS / 64];
    const int tid = threadIdx.x, b = blockIdx.z;
    const int tx0 = blockIdx.x * 64, ty0 = blockIdx.y * 16;
    const int cnt = paint_count(p.l, b);
    if (cnt <= 0) return;
    const int i = ty0 + (tid >> 4), j0 = tx0 + 4 * (tid & 15);
    const PaintGroup u = paint_group<0>(p.t, p.H, p.W, b, i, j0);
    const float ht = (float)p.s.thickness * 0.5f;
    const int alpha = p.s.fill_alpha;
    uint32_t px[4] = {0, 0, 0, 0};
    bool loaded = false, dirty = false;
    for (int hi = cnt - 1; hi >= 0; hi -= DR_THREADS) {
        const int n = draw_collect<false>(p, b, hi, tx0, ty0, 64, 16, hits, wave_cnt);
        if (n && u.nc) {
            if (!loaded) {
                loaded = true;
                paint_load(u, px);
            }
            for (int e = 0; e < n; ++e) {
                const DrawHit &h = hits[e];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    if (k >= u.nc) continue;
                    const int ops = draw_ops(h, p.s, ht, i, j0 + k);
                    if ((ops & 1) && alpha) { px[k] = draw_blend(px[k], h.col, alpha); dirty = true; }
                    if (ops & 2) { px[k] = h.col; dirty = true; }
                    if (ops & 4) { px[k] = (ops & 8) ? h.tcol : h.col; dirty = true; }
                }
            }
        }
        __syncthreads();                                                  // the list is rewritten by the next chunk
    }
    if (dirty) paint_store(u, px, paint_inside(u));
}

// PLANAR: U and V planes (I420) instead of one plane of pairs (NV12 / NV21)
template <bool PLANAR>
__global__ __launch_bounds__(DR_THREADS) void draw_yuv_kernel(const DrawArgs p) {
    __shared__ DrawHit hits[DR_THREADS];
    __shared__ int wave_cnt[DR_THREADS / 64];
    constexpr int FMT = PLANAR ? 2 : 1;
    const int tid = threadIdx.x, b = blockIdx.z;
    const int tx0 = blockIdx.x * 128, ty0 = blockIdx.y * 16;
    const int cnt = paint_count(p.l, b);
    if (cnt <= 0) return;
    const int i0 = ty0 + 2 * (tid >> 5), j0 = tx0 + 4 * (tid & 31);
    const PaintGroup u = paint_group<FMT>(p.t, p.H, p.W, b, i0, j0);
    const float ht = (float)p.s.thickness * 0.5f;
    const int alpha = p.s.fill_alpha;
    int Y[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}}, U[2] = {0, 0}, V[2] = {0, 0};
    bool loaded = false, dirty = false;
    for (int hi = cnt - 1; hi >= 0; hi -= DR_THREADS) {
        const int n = draw_collect<true>(p, b, hi, tx0, ty0, 128, 16, hits, wave_cnt);
        if (n && u.nc) {
            if (!loaded) {
                loaded = true;
                paint_load<FMT>(p.t, u, Y, U, V);
            }
            for (int e = 0; e < n; ++e) {
                const DrawHit &h = hits[e];
                const int cy = px_chan(h.col, 0), ty = px_chan(h.tcol, 0);
#pragma unroll
                for (int q = 0; q < 2; ++q) {
                    int any = 0;                                          // operations that hit a pixel of the quad
                    uint32_t lab = 0;                                     // the label's colour at the first pixel it hits
#pragma unroll
                    for (int r = 0; r < 2; ++r)
#pragma unroll
                        for (int k = 2 * q; k < 2 * q + 2; ++k) {
                            if (r >= u.nr || k >= u.nc) continue;
                            const int ops = draw_ops(h, p.s, ht, i0 + r, j0 + k);
                            if ((ops & 1) && alpha) Y[r][k] = draw_blend1(Y[r][k], cy, alpha);
                            if (ops & 2) Y[r][k] = cy;
                            if (ops & 4) {
                                Y[r][k] = (ops & 8) ? ty : cy;
                                if (!(any & 4)) lab = (ops & 8) ? h.tcol : h.col;
                            }
                            any |= ops;
                        }
                    if (!alpha) any &= ~1;
                    if (any & 1) { U[q] = draw_blend1(U[q], px_chan(h.col, 1), alpha); V[q] = draw_blend1(V[q], px_chan(h.col, 2), alpha); }
                    if (any & 2) { U[q] = px_chan(h.col, 1); V[q] = px_chan(h.col, 2); }
                    if (any & 4) { U[q] = px_chan(lab, 1); V[q] = px_chan(lab, 2); }
                    if (any & 7) dirty = true;
                }
            }
        }
        __syncthreads();                                                  // the list is rewritten by the next chunk
    }
    if (dirty) paint_store<FMT>(p.t, u, Y, U, V, paint_inside(u), paint_quads(paint_inside(u)));
}

// The checks both entry points share
int draw_check(const mydet_draw_list *l, const mydet_draw_style *s, int B, int H, int W) {
    if (!s || B <= 0 || H <= 0 || W <= 0 || paint_list_check(l, true)) return MYDET_E_BADARG;
    if (s->thickness < 1 || s->thickness > MYDET_DRAW_MAX_THICKNESS || s->fill_alpha < 0 || s->fill_alpha > 255) return MYDET_E_BADARG;
    if (s->color_mode != MYDET_DRAW_COLOR_CLASS && s->color_mode != MYDET_DRAW_COLOR_ID && s->color_mode != MYDET_DRAW_COLOR_FIXED)
        return MYDET_E_BADARG;
    if (s->color_mode != MYDET_DRAW_COLOR_FIXED && (!s->palette || s->n_palette < 1)) return MYDET_E_BADARG;
    if (s->label_flags & ~(MYDET_DRAW_LABEL_CLASS | MYDET_DRAW_LABEL_SCORE | MYDET_DRAW_LABEL_ID)) return MYDET_E_BADARG;
    if (s->label_flags && (!s->atlas || s->ch < 8 || s->ch > 64 || s->cw < 1 || s->cw > 64)) return MYDET_E_BADARG;
    if (s->names && s->n_names < 1) return MYDET_E_BADARG;
    return 0;
}

// The launch both entry points share: TW x 16 tiles over B frames of H x W
template <typename Kernel>
int draw_launch(Kernel kernel, DrawArgs &p, int TW, int B, int H, int W, const mydet_draw_list *list, const mydet_draw_style *style,
                void *stream) {
    const int gy = (H + 15) / 16;
    if (B > 65535 || gy > 65535) return MYDET_E_UNSUPP;
    p.l = *list; p.s = *style; p.H = H; p.W = W;
    const dim3 grid((unsigned)((W + TW - 1) / TW), (unsigned)gy, (unsigned)B);
    hipLaunchKernelGGL(kernel, grid, dim3(DR_THREADS), 0, (hipStream_t)stream, p);
    return mydet_launch_status();
}

}  // namespace

extern "C" int mydet_draw_boxes_rgb_u8(unsigned char *dst, int B, int H, int W, int64_t dst_img_bytes, int64_t dst_row_bytes,
                                       const mydet_draw_list *list, const mydet_draw_style *style, void *stream) {
    DrawArgs p = {};
    int code = draw_check(list, style, B, H, W);
    if (!code) code = paint_planes_rgb(p.t, dst, dst_img_bytes, dst_row_bytes, W);
    if (code) return code;
    return draw_launch(draw_rgb_kernel, p, 64, B, H, W, list, style, stream);
}

extern "C" int mydet_draw_boxes_yuv420_u8(const mydet_yuv420_src *planes, int B, int H, int W, const mydet_draw_list *list,
                                          const mydet_draw_style *style, void *stream) {
    DrawArgs p = {};
    int code = draw_check(list, style, B, H, W);
    if (!code) code = paint_planes_yuv420(p.t, planes, W);
    if (code) return code;
    p.k = DRAW_YUV[planes->matrix][planes->full_range];
    const bool planar = planes->layout == MYDET_YUV420_I420;
    return draw_launch(planar ? draw_yuv_kernel<true> : draw_yuv_kernel<false>, p, 128, B, H, W, list, style, stream);
}
