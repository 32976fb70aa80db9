"""Plain-Python restatement of the counting overlay's raster rules and of the trails ring (include/mydet.h: mydet_draw_overlay_*,
mydet_trails_frames), written from the rule text: Python integers for every geometric decision (no overflow to think about),
numpy only to hold masks and pixels.  Inside, q and the anchors come from tests/_zones_ref.py, the blend, the glyph bitmap and
the text colour from tests/_draw_ref.py.  tests/test_overlay_host.py holds it to exact fractions; tests/test_gpu_overlay.py holds
the kernels to it with ==."""
import math

import numpy as np

import _draw_ref as dr
import _zones_ref as zr
from mydetection_amd import ops

MAX_GLYPHS, NAME_CHARS, MAX_SHOWN = 40, 16, 999999
I64 = 1 << 63


def centre(i, j):
    return (16 * j + 8, 16 * i + 8)


# ------------------------------------------------------------------------------------------------------------------ strokes
def capsule_hit(a, b, t, p):
    """The centre p lies within t/2 pixels of the segment a -> b: the integer rule, Python ints."""
    dx, dy = b[0] - a[0], b[1] - a[1]
    vx, vy = p[0] - a[0], p[1] - a[1]
    len2, u, r = dx * dx + dy * dy, vx * dx + vy * dy, 8 * t
    if u <= 0:
        return vx * vx + vy * vy <= r * r
    if u >= len2:
        wx, wy = p[0] - b[0], p[1] - b[1]
        return wx * wx + wy * wy <= r * r
    c = dx * vy - dy * vx
    return c * c <= r * r * len2


def capsule_hit_i64(a, b, t, p):
    """The same decision as a kernel in int64 takes it: every intermediate is asserted to fit, |cross| >= 2^31 is rejected first."""
    def fits(v):
        assert -I64 <= v < I64, v
        return v
    dx, dy = b[0] - a[0], b[1] - a[1]
    vx, vy = p[0] - a[0], p[1] - a[1]
    assert max(abs(dx), abs(dy)) <= 1 << 21 and max(abs(vx), abs(vy)) < 1 << 21
    len2, u, r2 = fits(dx * dx + dy * dy), fits(vx * dx + vy * dy), (8 * t) ** 2
    if u <= 0:
        return fits(vx * vx + vy * vy) <= r2
    if u >= len2:
        wx, wy = vx - dx, vy - dy
        return fits(wx * wx + wy * wy) <= r2
    c = fits(dx * vy - dy * vx)
    if abs(c) >= 1 << 31:
        return False
    return fits(c * c) <= fits(r2 * len2)


def capsule_mask(H, W, a, b, t):
    """bool [H, W]: the pixels the stroke a -> b of thickness t paints (only the bounding box is visited)."""
    m = np.zeros((H, W), dtype=bool)
    r = 8 * t
    j_lo, j_hi = max(0, (min(a[0], b[0]) - r - 8) // 16), min(W - 1, (max(a[0], b[0]) + r) // 16)
    i_lo, i_hi = max(0, (min(a[1], b[1]) - r - 8) // 16), min(H - 1, (max(a[1], b[1]) + r) // 16)
    for i in range(i_lo, i_hi + 1):
        for j in range(j_lo, j_hi + 1):
            m[i, j] = capsule_hit(a, b, t, centre(i, j))
    return m


def fill_mask(H, W, poly):
    """bool [H, W]: the pixels whose centres are inside the quantised polygon by _zones_ref.inside."""
    m = np.zeros((H, W), dtype=bool)
    ys, xs = [p[1] for p in poly], [p[0] for p in poly]
    for i in range(max(0, (min(ys) - 8) // 16), min(H - 1, max(ys) // 16) + 1):
        for j in range(max(0, (min(xs) - 8) // 16), min(W - 1, max(xs) // 16) + 1):
            m[i, j] = zr.inside(poly, centre(i, j))
    return m


def tick(line, thickness):
    """((M.x, M.y), (E.x, E.y)) of the quantised line (A, B)."""
    (ax, ay), (bx, by) = line
    m = ((ax + bx) >> 1, (ay + by) >> 1)
    n = (-(by - ay), bx - ax)
    lh = math.isqrt(n[0] * n[0] + n[1] * n[1])
    k = 16 * 4 * thickness
    e = tuple(m[c] + (abs(n[c] * k) // lh) * (1 if n[c] >= 0 else -1) for c in range(2))
    return m, e


# ------------------------------------------------------------------------------------------------------------------- labels
def shown(v):
    return str(min(int(v), MAX_SHOWN))


def zone_text(name, counters, occupancy, entries, visits):
    text = name[:NAME_CHARS]
    if 'occupancy' in counters:
        text += ' ' + shown(occupancy)
    if 'entries' in counters:
        text += ' +' + shown(entries)
    if 'visits' in counters:
        text += ' -' + shown(visits)
    return text[:MAX_GLYPHS]


def line_text(name, pos, neg):
    return f'{name[:NAME_CHARS]} +{shown(pos)} -{shown(neg)}'[:MAX_GLYPHS]


def label_rect(H, W, anchor, n, ch, cw):
    """(left, top) of a label of n glyphs at the fixed-point anchor."""
    left = min(max(anchor[0] >> 4, 0), max(0, W - n * cw))
    top = min(max((anchor[1] >> 4) - ch, 0), max(0, H - ch))
    return left, top


def label_masks(H, W, anchor, text, atlas):
    lab, txt = np.zeros((H, W), dtype=bool), np.zeros((H, W), dtype=bool)
    if not text:
        return lab, txt
    codes = [ord(c) if 32 <= ord(c) <= 127 else ord('?') for c in text]
    bm = np.concatenate([atlas[c - 32] for c in codes], axis=1) != 0
    ch, lw = bm.shape
    left, top = label_rect(H, W, anchor, len(text), ch, atlas.shape[2])
    hh, ww = min(ch, H - top), min(lw, W - left)
    lab[top:top + hh, left:left + ww] = True
    txt[top:top + hh, left:left + ww] = bm[:hh, :ww]
    return lab, txt


# ------------------------------------------------------------------------------------------------------------------- trails
class TrailStream:
    """The trail state of one stream: per slot the id, the ring of the last L quantised anchors, its fill and its head."""

    def __init__(self, max_tracks, L, anchor='center', classes=None):
        self.L, self.mt = L, max_tracks
        self.zs = zr.ZoneSet((1, 1), anchor=anchor)                    # anchor_of alone is used
        self.classes = None if classes is None else set(int(c) for c in classes)
        self.id = [0] * max_tracks
        self.fill, self.head = [0] * max_tracks, [0] * max_tracks
        self.ring = [[(0, 0)] * L for _ in range(max_tracks)]

    def frame(self, box, ids, cls, missed, count):
        """One frame; returns (points [MT][L][2], len [MT], bbox [MT][4]) as lists."""
        L = self.L
        points, lens, bboxes = [], [], []
        for t in range(self.mt):
            tid = int(ids[t])
            if count >= 0:                                               # 1. a bad-class frame leaves the state alone
                if self.id[t] != 0 and self.id[t] != tid:                # 2. clear
                    self.id[t], self.fill[t], self.head[t], self.ring[t] = 0, 0, 0, [(0, 0)] * L
                if tid != 0 and missed[t] == 0 and (self.classes is None or int(cls[t]) in self.classes):
                    p = self.zs.anchor_of(box[t])                        # 3. push
                    if p is not None:
                        if self.id[t] == 0:
                            self.id[t] = tid
                        self.ring[t][self.head[t]] = p
                        self.head[t] = (self.head[t] + 1) % L
                        self.fill[t] = min(self.fill[t] + 1, L)
            pts = [self.ring[t][(self.head[t] - 1 - k) % L] for k in range(self.fill[t])]   # 4. newest first
            points.append([list(p) for p in pts] + [[0, 0]] * (L - len(pts)))
            lens.append(self.fill[t] if self.id[t] == tid else 0)
            bboxes.append([min(p[0] for p in pts), min(p[1] for p in pts), max(p[0] for p in pts), max(p[1] for p in pts)] if pts else [0] * 4)
        return points, lens, bboxes

    def arrays(self):
        """The state as ops.trails_state_views names it (one stream)."""
        return {'id': np.array(self.id, np.int64), 'fill': np.array(self.fill, np.int32), 'head': np.array(self.head, np.int32),
                'ring': np.array(self.ring, np.int32).reshape(self.mt, self.L, 2)}


def run_trails(streams, track_out):
    """F frames of every stream (track_out as in _zones_ref.run); returns points [S,F,MT,L,2], len [S,F,MT], bbox [S,F,MT,4] int32."""
    S, F, MT = track_out['id'].shape
    L = streams[0].L
    out = {'points': np.zeros((S, F, MT, L, 2), np.int32), 'len': np.zeros((S, F, MT), np.int32), 'bbox': np.zeros((S, F, MT, 4), np.int32)}
    for s in range(S):
        for f in range(F):
            r = streams[s].frame(track_out['box'][s, f], track_out['id'][s, f], track_out['cls'][s, f], track_out['missed'][s, f],
                                 int(track_out['count'][s, f]))
            out['points'][s, f], out['len'][s, f], out['bbox'][s, f] = r
    return out


# ------------------------------------------------------------------------------------------------------------------ painting
def frame_ops(scene, o, H, W):
    """The operations of frame o in paint order: ('blend', mask, rgb, alpha) | ('set', mask, rgb) | ('label', lab, txt, rgb).
    scene: a dict -- polygons, lines (quantised), names, thickness, zones, lines_on, counters, zone_alpha, occupied_alpha,
    n_palette, label_height; per frame occupancy [B][Z], zone_counts [B][Z][4], line_counts [B][L][2]; trails: None or a dict
    of points [B][MT][L][2], len, id, missed [B][MT], thickness, coasting."""
    pal = ops.draw_palette(scene['n_palette'])
    out = []
    polys = scene['polygons'] if scene['zones'] else []
    lines = scene['lines'] if scene['lines_on'] else []
    t = scene['thickness']
    for z, poly in enumerate(polys):
        alpha = scene['zone_alpha'] if scene['occupancy'][o][z] == 0 else scene['occupied_alpha']
        if alpha:
            out.append(('blend', fill_mask(H, W, poly), pal[z % len(pal)], alpha))
    for z, poly in enumerate(polys):
        for e in range(len(poly)):
            out.append(('set', capsule_mask(H, W, poly[e], poly[(e + 1) % len(poly)], t), pal[z % len(pal)]))
    for l, line in enumerate(lines):
        out.append(('set', capsule_mask(H, W, line[0], line[1], t), pal[l % len(pal)]))
        m, e = tick(line, t)
        out.append(('set', capsule_mask(H, W, m, e, t), pal[l % len(pal)]))
    tr = scene.get('trails')
    if tr is not None:
        for slot in range(len(tr['len'][o])):
            n, ms = int(tr['len'][o][slot]), int(tr['missed'][o][slot])
            if n >= 2 and (ms == 0 or (tr['coasting'] and ms >= 0)):
                col = pal[int(tr['id'][o][slot]) % len(pal)]
                pts = [tuple(int(v) for v in p) for p in tr['points'][o][slot][:n]]
                for k in range(n - 1):
                    out.append(('set', capsule_mask(H, W, pts[k], pts[k + 1], tr['thickness']), col))
    if scene['counters']:
        atlas = ops.glyph_atlas(scene['label_height']).numpy()
        for z, poly in enumerate(polys):
            e, _, _, v = (int(c) for c in scene['zone_counts'][o][z])
            text = zone_text(scene['names'][z], scene['counters'], scene['occupancy'][o][z], e, v)
            anchor = min(poly, key=lambda p: (p[1], p[0]))
            out.append(('label',) + label_masks(H, W, anchor, text, atlas) + (pal[z % len(pal)],))
        for l, line in enumerate(lines):
            pos, neg = (int(c) for c in scene['line_counts'][o][l])
            text = line_text(scene['names'][len(scene['polygons']) + l], pos, neg)
            out.append(('label',) + label_masks(H, W, tick(line, t)[0], text, atlas) + (pal[l % len(pal)],))
    return out


def paint_rgb(img, oplist):
    """Apply the operations to one frame [H, W, 3] uint8 in place."""
    for op in oplist:
        if op[0] == 'blend':
            _, m, col, alpha = op
            for c in range(3):
                img[..., c][m] = dr.blend(img[..., c][m], col[c], alpha)
        elif op[0] == 'set':
            img[op[1]] = op[2]
        else:
            _, lab, txt, col = op
            img[lab] = col
            img[txt] = dr.text_color(col)


def paint_yuv(Y, U, V, oplist, matrix='bt601', full_range=False):
    """Apply the operations to one 4:2:0 frame in place: Y [H, W], U and V [ceil(H/2), ceil(W/2)] uint8.  A chroma sample takes
    every operation that hits a pixel of its quad, once, in paint order."""
    H, W = Y.shape
    H2, W2 = U.shape

    def quads(mask):
        m = np.zeros((2 * H2, 2 * W2), dtype=bool)
        m[:H, :W] = mask
        return m.reshape(H2, 2, W2, 2)

    def yuv(rgb):
        return tuple(int(v) for v in ops.rgb_to_yuv(np.asarray(rgb, dtype=np.uint8), matrix, full_range))

    for op in oplist:
        if op[0] == 'blend':
            _, m, col, alpha = op
            cy, cu, cv = yuv(col)
            Y[m] = dr.blend(Y[m], cy, alpha)
            q = quads(m).any(axis=(1, 3))
            U[q], V[q] = dr.blend(U[q], cu, alpha), dr.blend(V[q], cv, alpha)
        elif op[0] == 'set':
            cy, cu, cv = yuv(op[2])
            Y[op[1]] = cy
            q = quads(op[1]).any(axis=(1, 3))
            U[q], V[q] = cu, cv
        else:
            _, lab, txt, col = op
            (cy, cu, cv), (ty, tu, tv) = yuv(col), yuv(dr.text_color(col))
            Y[lab] = cy
            Y[txt] = ty
            ql, qt = quads(lab), quads(txt)
            done = np.zeros((H2, W2), dtype=bool)
            for r in range(2):                                           # the colour at the first pixel of the quad the label hits
                for c in range(2):
                    first = ql[:, r, :, c] & ~done
                    is_text = first & qt[:, r, :, c]
                    U[first], V[first] = cu, cv
                    U[is_text], V[is_text] = tu, tv
                    done |= first
