// Overlay renderer: outlines of axis-aligned and rotated boxes, translucent fills and text labels painted IN PLACE into uint8
// RGB frames or into the planes of the 8-bit 4:2:0 layouts, one launch per batch (include/mydet.h: mydet_draw_boxes_rgb_u8,
// mydet_draw_boxes_yuv420_u8, where the raster rules are; DESIGN.md has them too).  Built with -ffp-contract=off: the
// thresholds of the rules are float32 expressions that must not be fused.
//
// One workgroup of 256 lanes per image tile.  RGB: 64 x 16 pixels, a lane owns 4 neighbouring pixels of a row (12 bytes).
// 4:2:0: 128 x 16 pixels, a lane owns two neighbouring chroma quads (4 x 2 luma pixels + 2 chroma samples), so luma and chroma
// come from one evaluation.  The frame's rows are walked in paint order (count - 1 down to 0) in chunks of 256: every lane tests
// one row against the tile -- the bounding box of the outer rectangle, one pixel wider, less (without a fill) the tiles that lie
// inside the outline's hole, united with the label rectangle -- and the
// hits are compacted in paint order into LDS (geometry, colours, label text: 84 bytes each, 21 KiB).  A tile without a hit in
// any chunk reads and writes no pixel.  The others load their pixels once, walk the short list per pixel and store the pixel
// groups that changed: with dword stores when address, pitch and frame stride allow (see the header), byte by byte otherwise.
#include "box_rot.h"
#include "draw_yuv.h"
#include "pixel_math.h"

namespace {

constexpr int DR_THREADS = 256;
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
    unsigned char *p[3];                     // RGB: p[0] = the frames.  4:2:0: Y; interleaved chroma or U; V
    int64_t img[3], row[3];                  // bytes between frames / rows
    int wide[3];                             // the plane takes the dword (planar chroma: 16-bit) accesses
    int v_first;                             // NV21: the pair is (V, U)
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
    const int tid = threadIdx.x, r = hi - tid;
    const mydet_draw_list &l = p.l;
    const float ht = (float)p.s.thickness * 0.5f;
    bool hit = false;
    float cx = 0, cy = 0, w = 0, h = 0, c = 1.0f, s = 0.0f;
    int lx = 0, ly = 0, lw = 0;
    if (r >= 0) {
        const float *bx = l.box + (int64_t)b * l.box_frame_stride + (int64_t)r * l.box_row_stride;
        cx = bx[0]; cy = bx[1]; w = bx[2]; h = bx[3];
        const float ang = l.angle ? l.angle[(int64_t)b * l.angle_frame_stride + (int64_t)r * l.angle_row_stride] : 0.0f;
        const bool ok = isfinite(cx) && isfinite(cy) && isfinite(w) && isfinite(h) && isfinite(ang) && w > 0.0f && h > 0.0f;
        if (ok) {
            box_rotation<false>(ang, c, s);
            const float ow = w * 0.5f + ht, oh = h * 0.5f + ht;
            const float ex = fabsf(c) * ow + fabsf(s) * oh + 1.0f, ey = fabsf(s) * ow + fabsf(c) * oh + 1.0f;
            hit = !(cx - ex > (float)(tx0 + TW) || cx + ex < (float)tx0 || cy - ey > (float)(ty0 + TH) || cy + ey < (float)ty0);
            if (hit && p.s.fill_alpha == 0) {                             // no fill: a tile inside the outline's hole is not hit
                const float iw = w * 0.5f - ht - 1.0f, ih = h * 0.5f - ht - 1.0f;    // the hole, one pixel smaller
                bool inside = true;
#pragma unroll
                for (int k = 0; k < 4; ++k) {                             // the hole is convex: the four corners decide
                    const float dx = (float)(tx0 + (k & 1) * TW) - cx, dy = (float)(ty0 + (k >> 1) * TH) - cy;
                    inside = inside && fabsf(dx * c + dy * s) < iw && fabsf(dy * c - dx * s) < ih;
                }
                hit = !inside;
            }
            if (p.s.label_flags) {                                        // the label rectangle needs the glyph count alone
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
    }
    const unsigned long long m = __ballot(hit);
    const int lane = tid & 63, wv = tid >> 6;
    if (lane == 0) wave_cnt[wv] = __popcll(m);
    __syncthreads();
    int base = 0, total = 0;
    for (int k = 0; k < DR_THREADS / 64; ++k) {
        const int n = wave_cnt[k];
        if (k < wv) base += n;
        total += n;
    }
    if (hit) {
        DrawHit &o = hits[base + __popcll(m & ((1ull << lane) - 1ull))];
        o.cx = cx; o.cy = cy; o.hw = w * 0.5f; o.hh = h * 0.5f; o.c = c; o.s = s;
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
    }
    __syncthreads();
    return total;
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
    int cnt = p.l.count ? p.l.count[(int64_t)b * p.l.count_stride] : p.l.K;
    if (cnt <= 0) return;
    cnt = min(cnt, p.l.K);
    const int i = ty0 + (tid >> 4), j0 = tx0 + 4 * (tid & 15);
    const int nv = i < p.H ? px_clamp(p.W - j0, 0, 4) : 0;               // this lane's pixels inside the frame
    unsigned char *o = p.p[0] + (int64_t)b * p.img[0] + (int64_t)i * p.row[0] + (int64_t)j0 * 3;
    const bool words = p.wide[0] && nv == 4;
    const float ht = (float)p.s.thickness * 0.5f;
    const int alpha = p.s.fill_alpha;
    uint32_t px[4] = {0, 0, 0, 0};
    bool loaded = false, dirty = false;
    for (int hi = cnt - 1; hi >= 0; hi -= DR_THREADS) {
        const int n = draw_collect<false>(p, b, hi, tx0, ty0, 64, 16, hits, wave_cnt);
        if (n && nv) {
            if (!loaded) {
                loaded = true;
                if (words) {
                    const uint32_t *o4 = reinterpret_cast<const uint32_t *>(o);
                    const uint32_t w0 = o4[0], w1 = o4[1], w2 = o4[2];
                    px[0] = w0 & 0xffffffu; px[1] = (w0 >> 24) | ((w1 & 0xffffu) << 8); px[2] = (w1 >> 16) | ((w2 & 0xffu) << 16); px[3] = w2 >> 8;
                } else {
                    for (int k = 0; k < nv; ++k) px[k] = px_pack(o[3 * k], o[3 * k + 1], o[3 * k + 2]);
                }
            }
            for (int e = 0; e < n; ++e) {
                const DrawHit &h = hits[e];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    if (k >= nv) continue;
                    const int ops = draw_ops(h, p.s, ht, i, j0 + k);
                    if ((ops & 1) && alpha) { px[k] = draw_blend(px[k], h.col, alpha); dirty = true; }
                    if (ops & 2) { px[k] = h.col; dirty = true; }
                    if (ops & 4) { px[k] = (ops & 8) ? h.tcol : h.col; dirty = true; }
                }
            }
        }
        __syncthreads();                                                  // the list is rewritten by the next chunk
    }
    if (!dirty) return;
    if (words) {
        uint32_t *o4 = reinterpret_cast<uint32_t *>(o);
        o4[0] = px[0] | (px[1] << 24);
        o4[1] = (px[1] >> 8) | (px[2] << 16);
        o4[2] = (px[2] >> 16) | (px[3] << 8);
    } else {
        for (int k = 0; k < nv; ++k) {
            o[3 * k] = (unsigned char)px[k]; o[3 * k + 1] = (unsigned char)(px[k] >> 8); o[3 * k + 2] = (unsigned char)(px[k] >> 16);
        }
    }
}

// PLANAR: U and V planes (I420) instead of one plane of pairs (NV12 / NV21)
template <bool PLANAR>
__global__ __launch_bounds__(DR_THREADS) void draw_yuv_kernel(const DrawArgs p) {
    __shared__ DrawHit hits[DR_THREADS];
    __shared__ int wave_cnt[DR_THREADS / 64];
    const int tid = threadIdx.x, b = blockIdx.z;
    const int tx0 = blockIdx.x * 128, ty0 = blockIdx.y * 16;
    int cnt = p.l.count ? p.l.count[(int64_t)b * p.l.count_stride] : p.l.K;
    if (cnt <= 0) return;
    cnt = min(cnt, p.l.K);
    const int i0 = ty0 + 2 * (tid >> 5), j0 = tx0 + 4 * (tid & 31);       // two quads: rows i0, i0 + 1, columns j0 .. j0 + 3
    const int nr = px_clamp(p.H - i0, 0, 2), nc = nr ? px_clamp(p.W - j0, 0, 4) : 0;
    const int nq = (nc + 1) >> 1;                                        // chroma samples of this lane
    const int cw = (p.W + 1) >> 1;
    unsigned char *yo = p.p[0] + (int64_t)b * p.img[0] + (int64_t)i0 * p.row[0] + j0;
    unsigned char *uo, *vo = nullptr;                                    // interleaved: uo = the pair of the first quad
    if (PLANAR) {
        uo = p.p[1] + (int64_t)b * p.img[1] + (int64_t)(i0 >> 1) * p.row[1] + (j0 >> 1);
        vo = p.p[2] + (int64_t)b * p.img[2] + (int64_t)(i0 >> 1) * p.row[2] + (j0 >> 1);
    } else {
        uo = p.p[1] + (int64_t)b * p.img[1] + (int64_t)(i0 >> 1) * p.row[1] + j0;
    }
    const bool ywords = p.wide[0] && nc == 4;
    const bool cwords = nq == 2 && (j0 >> 1) + 2 <= cw && (PLANAR ? (p.wide[1] && p.wide[2]) : p.wide[1]);
    const int su = p.v_first ? 1 : 0;                                    // byte of U inside an interleaved pair
    const float ht = (float)p.s.thickness * 0.5f;
    const int alpha = p.s.fill_alpha;
    int Y[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}}, U[2] = {0, 0}, V[2] = {0, 0};
    bool loaded = false, dirty = false;
    for (int hi = cnt - 1; hi >= 0; hi -= DR_THREADS) {
        const int n = draw_collect<true>(p, b, hi, tx0, ty0, 128, 16, hits, wave_cnt);
        if (n && nc) {
            if (!loaded) {
                loaded = true;
                for (int r = 0; r < nr; ++r) {
                    const unsigned char *yr = yo + (int64_t)r * p.row[0];
                    if (ywords) {
                        const uint32_t w = *reinterpret_cast<const uint32_t *>(yr);
#pragma unroll
                        for (int k = 0; k < 4; ++k) Y[r][k] = (int)((w >> (8 * k)) & 255u);
                    } else {
#pragma unroll
                        for (int k = 0; k < 4; ++k) if (k < nc) Y[r][k] = yr[k];
                    }
                }
                if (PLANAR) {
                    if (cwords) {
                        const uint32_t u = *reinterpret_cast<const uint16_t *>(uo), v = *reinterpret_cast<const uint16_t *>(vo);
                        U[0] = u & 255u; U[1] = u >> 8; V[0] = v & 255u; V[1] = v >> 8;
                    } else {
                        for (int q = 0; q < nq; ++q) { U[q] = uo[q]; V[q] = vo[q]; }
                    }
                } else {
                    if (cwords) {
                        const uint32_t w = *reinterpret_cast<const uint32_t *>(uo);
                        U[0] = (w >> (8 * su)) & 255u; V[0] = (w >> (8 * (1 - su))) & 255u;
                        U[1] = (w >> (16 + 8 * su)) & 255u; V[1] = (w >> (16 + 8 * (1 - su))) & 255u;
                    } else {
                        for (int q = 0; q < nq; ++q) { U[q] = uo[2 * q + su]; V[q] = uo[2 * q + 1 - su]; }
                    }
                }
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
                            if (r >= nr || k >= nc) continue;
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
    if (!dirty) return;
    for (int r = 0; r < nr; ++r) {
        unsigned char *yr = yo + (int64_t)r * p.row[0];
        if (ywords) {
            *reinterpret_cast<uint32_t *>(yr) = (uint32_t)Y[r][0] | ((uint32_t)Y[r][1] << 8) | ((uint32_t)Y[r][2] << 16) | ((uint32_t)Y[r][3] << 24);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) if (k < nc) yr[k] = (unsigned char)Y[r][k];
        }
    }
    if (PLANAR) {
        if (cwords) {
            *reinterpret_cast<uint16_t *>(uo) = (uint16_t)(U[0] | (U[1] << 8));
            *reinterpret_cast<uint16_t *>(vo) = (uint16_t)(V[0] | (V[1] << 8));
        } else {
            for (int q = 0; q < nq; ++q) { uo[q] = (unsigned char)U[q]; vo[q] = (unsigned char)V[q]; }
        }
    } else {
        if (cwords) {
            const uint32_t p0 = (uint32_t)(su ? (V[0] | (U[0] << 8)) : (U[0] | (V[0] << 8)));
            const uint32_t p1 = (uint32_t)(su ? (V[1] | (U[1] << 8)) : (U[1] | (V[1] << 8)));
            *reinterpret_cast<uint32_t *>(uo) = p0 | (p1 << 16);
        } else {
            for (int q = 0; q < nq; ++q) { uo[2 * q + su] = (unsigned char)U[q]; uo[2 * q + 1 - su] = (unsigned char)V[q]; }
        }
    }
}

// The checks both entry points share
int draw_check(const mydet_draw_list *l, const mydet_draw_style *s, int B, int H, int W) {
    if (!l || !s || B <= 0 || H <= 0 || W <= 0) return MYDET_E_BADARG;
    if (!l->box || l->K < 1 || l->K > MYDET_DRAW_MAX_BOXES) return MYDET_E_BADARG;
    const int64_t strides[] = {l->box_frame_stride, l->box_row_stride, l->angle_frame_stride, l->angle_row_stride, l->score_frame_stride,
                               l->score_row_stride, l->cls_frame_stride, l->cls_row_stride, l->id_frame_stride, l->id_row_stride,
                               l->count_stride};
    for (int64_t v : strides)
        if (v < 0) return MYDET_E_BADARG;
    if (s->thickness < 1 || s->thickness > MYDET_DRAW_MAX_THICKNESS || s->fill_alpha < 0 || s->fill_alpha > 255) return MYDET_E_BADARG;
    if (s->color_mode != MYDET_DRAW_COLOR_CLASS && s->color_mode != MYDET_DRAW_COLOR_ID && s->color_mode != MYDET_DRAW_COLOR_FIXED)
        return MYDET_E_BADARG;
    if (s->color_mode != MYDET_DRAW_COLOR_FIXED && (!s->palette || s->n_palette < 1)) return MYDET_E_BADARG;
    if (s->label_flags & ~(MYDET_DRAW_LABEL_CLASS | MYDET_DRAW_LABEL_SCORE | MYDET_DRAW_LABEL_ID)) return MYDET_E_BADARG;
    if (s->label_flags && (!s->atlas || s->ch < 8 || s->ch > 64 || s->cw < 1 || s->cw > 64)) return MYDET_E_BADARG;
    if (s->names && s->n_names < 1) return MYDET_E_BADARG;
    return 0;
}

}  // namespace

extern "C" int mydet_draw_boxes_rgb_u8(unsigned char *dst, int B, int H, int W, int64_t dst_img_bytes, int64_t dst_row_bytes,
                                       const mydet_draw_list *list, const mydet_draw_style *style, void *stream) {
    const int code = draw_check(list, style, B, H, W);
    if (code) return code;
    if (!dst || dst_row_bytes < (int64_t)W * 3 || dst_img_bytes < 0) return MYDET_E_BADARG;
    const int gy = (H + 15) / 16;
    if (B > 65535 || gy > 65535) return MYDET_E_UNSUPP;
    DrawArgs p = {};
    p.l = *list; p.s = *style; p.H = H; p.W = W;
    p.p[0] = dst; p.img[0] = dst_img_bytes; p.row[0] = dst_row_bytes;
    p.wide[0] = (((uintptr_t)dst | (uintptr_t)dst_img_bytes | (uintptr_t)dst_row_bytes) & 3) == 0;
    const dim3 grid((unsigned)((W + 63) / 64), (unsigned)gy, (unsigned)B);
    hipLaunchKernelGGL(draw_rgb_kernel, grid, dim3(DR_THREADS), 0, (hipStream_t)stream, p);
    return mydet_launch_status();
}

extern "C" int mydet_draw_boxes_yuv420_u8(const mydet_yuv420_src *planes, int B, int H, int W, const mydet_draw_list *list,
                                          const mydet_draw_style *style, void *stream) {
    const int code = draw_check(list, style, B, H, W);
    if (code) return code;
    if (!planes || !planes->plane[0] || !planes->plane[1]) return MYDET_E_BADARG;
    if (planes->layout != MYDET_YUV420_NV12 && planes->layout != MYDET_YUV420_NV21 && planes->layout != MYDET_YUV420_I420)
        return MYDET_E_BADARG;                                            // unknown, or a 10-bit layout
    if (planes->matrix < 0 || planes->matrix > 1 || planes->full_range < 0 || planes->full_range > 1) return MYDET_E_BADARG;
    const bool planar = planes->layout == MYDET_YUV420_I420;
    if ((planes->plane[2] != nullptr) != planar) return MYDET_E_BADARG;
    const int64_t cw = ((int64_t)W + 1) / 2;
    const int64_t need[3] = {(int64_t)W, planar ? cw : 2 * cw, cw};
    const int wide[3] = {4, planar ? 2 : 4, 2};
    DrawArgs p = {};
    for (int i = 0; i < (planar ? 3 : 2); ++i) {
        if (planes->row_bytes[i] < need[i] || planes->img_bytes[i] < 0) return MYDET_E_BADARG;
        const uintptr_t bits = (uintptr_t)planes->plane[i] | (uintptr_t)planes->row_bytes[i] | (uintptr_t)planes->img_bytes[i];
        p.p[i] = static_cast<unsigned char *>(const_cast<void *>(planes->plane[i]));
        p.img[i] = planes->img_bytes[i]; p.row[i] = planes->row_bytes[i];
        p.wide[i] = (bits & (uintptr_t)(wide[i] - 1)) == 0;
    }
    const int gy = (H + 15) / 16;
    if (B > 65535 || gy > 65535) return MYDET_E_UNSUPP;
    p.l = *list; p.s = *style; p.H = H; p.W = W;
    p.v_first = planes->layout == MYDET_YUV420_NV21;
    p.k = DRAW_YUV[planes->matrix][planes->full_range];
    const dim3 grid((unsigned)((W + 127) / 128), (unsigned)gy, (unsigned)B);
    if (planar) hipLaunchKernelGGL(draw_yuv_kernel<true>, grid, dim3(DR_THREADS), 0, (hipStream_t)stream, p);
    else hipLaunchKernelGGL(draw_yuv_kernel<false>, grid, dim3(DR_THREADS), 0, (hipStream_t)stream, p);
    return mydet_launch_status();
}
