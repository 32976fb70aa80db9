"""Host tests of the counting overlay: the restatement tests/_overlay_ref.py is held to exact arithmetic (fractions), the host
functions of ops (ticks, anchors, label texts) to the restatement and to numbers derived by hand, and every argument rule of
ops.* and api.Overlay is raised with no device touched.  No GPU."""
import math
import os
import random
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

import _overlay_cases as oc
import _overlay_ref as ref
import _zones_ref as zr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COORD_MAX, FRAME_MAX = 1 << 20, 32768


def exact_hit(a, b, t, p):
    """The rule in words: the distance from p to the segment is at most t/2 pixels = 8t units; exact fractions."""
    d = (b[0] - a[0], b[1] - a[1])
    len2 = d[0] * d[0] + d[1] * d[1]
    s = Fraction(0) if len2 == 0 else min(max(Fraction((p[0] - a[0]) * d[0] + (p[1] - a[1]) * d[1], len2), Fraction(0)), Fraction(1))
    cx, cy = a[0] + s * d[0], a[1] + s * d[1]
    return (p[0] - cx) ** 2 + (p[1] - cy) ** 2 <= Fraction(8 * t) ** 2


def lattice(i_lo, i_hi, j_lo, j_hi):
    return [ref.centre(i, j) for i in range(i_lo, i_hi) for j in range(j_lo, j_hi)]


SEGMENTS = [
    ((8, 8), (168, 8), 2),                    # through pixel centres: the centres one row away are exactly at distance t/2
    ((8, 8), (168, 8), 1),
    ((0, 16), (160, 16), 1),                  # along a pixel boundary: both neighbouring rows at distance exactly t/2
    ((16, 0), (16, 160), 3),
    ((40, 40), (40, 40), 1),                  # a == b: a dot; (40, 40) is a centre's (8, 8) + (32, 32)
    ((40, 40), (40, 40), 4),
    ((8, 8), (104, 136), 2),                  # a 3-4-5 direction: centres at rational distance exactly t/2 exist
    ((-37, 91), (203, -14), 5),
    ((100, 100), (101, 100), 64),
]


def test_capsule_rule_equals_exact_distances():
    boundary = 0
    for a, b, t in SEGMENTS:
        for p in lattice(-6, 16, -6, 18):
            want = exact_hit(a, b, t, p)
            assert ref.capsule_hit(a, b, t, p) == want == ref.capsule_hit_i64(a, b, t, p), (a, b, t, p)
            d = (b[0] - a[0], b[1] - a[1])
            if d == (160, 0) and a[0] <= p[0] <= b[0] and abs(p[1] - a[1]) == 8 * t:
                boundary += 1
                assert want                                              # exactly at distance t/2: painted
    assert boundary > 0
    # the 3-4-5 segment: the centre (8 + 4*16, 8 - 3*16) lies on the normal through a at distance 5 * 16 = 80 = 8 * 10
    a, b = (8, 8), (104, 136)
    p = (8 + 64, 8 - 48)
    assert (p[0] - 8) * 96 + (p[1] - 8) * 128 == 0 and exact_hit(a, b, 10, p) and not exact_hit(a, b, 9, p)
    assert ref.capsule_hit(a, b, 10, p) and not ref.capsule_hit(a, b, 9, p)
    # capsule_mask visits the bounding box only: the same set as the rule at every centre of the frame
    for a, b, t in SEGMENTS[:4] + SEGMENTS[6:8]:
        m = ref.capsule_mask(14, 15, a, b, t)
        assert all(m[i, j] == ref.capsule_hit(a, b, t, ref.centre(i, j)) for i in range(14) for j in range(15))


def test_guarded_int64_form_equals_python_ints_at_the_limits():
    """The longest segment the limits allow, and seeded ones at the coordinate limits: every intermediate of the guarded form fits
    int64 (asserted inside) and the decision is that of unbounded integers; |cross| >= 2^31 occurs and is outside."""
    a, b = (-COORD_MAX, -COORD_MAX), (COORD_MAX, COORD_MAX)
    far = 16 * (FRAME_MAX - 1) + 8
    guarded = 0
    for p in [(8, 8), (far, far), (far, 8), (8, far), (far - 16, far), (24, 8)]:
        for t in (1, 64):
            assert ref.capsule_hit_i64(a, b, t, p) == ref.capsule_hit(a, b, t, p) == exact_hit(a, b, t, p)
    rng = random.Random(7)
    for _ in range(3000):
        edge = lambda: rng.choice([-COORD_MAX, COORD_MAX, rng.randint(-COORD_MAX, COORD_MAX)])          # noqa: E731
        a, b = (edge(), edge()), (edge(), edge())
        p = ref.centre(rng.choice([0, FRAME_MAX - 1, rng.randrange(FRAME_MAX)]), rng.choice([0, FRAME_MAX - 1, rng.randrange(FRAME_MAX)]))
        t = rng.choice([1, 2, 64])
        d, v = (b[0] - a[0], b[1] - a[1]), (p[0] - a[0], p[1] - a[1])
        if 0 < v[0] * d[0] + v[1] * d[1] < d[0] * d[0] + d[1] * d[1] and abs(d[0] * v[1] - d[1] * v[0]) >= 1 << 31:
            guarded += 1
        assert ref.capsule_hit_i64(a, b, t, p) == ref.capsule_hit(a, b, t, p), (a, b, t, p)
    assert guarded > 100
    # near misses and hits around a long segment: points chosen next to it
    a, b = (-COORD_MAX, 3), (COORD_MAX, 5)
    for j in range(0, FRAME_MAX, 997):
        for i in range(0, 6):
            p = ref.centre(i, j)
            assert ref.capsule_hit_i64(a, b, 2, p) == ref.capsule_hit(a, b, 2, p) == exact_hit(a, b, 2, p)


def test_fill_mask_is_the_zones_inside_rule_and_shared_edges_split_the_pixels():
    H, W = 37, 70
    polys = [zr.quantise(p) for p in oc.POLYGONS]
    for poly in polys:
        m = ref.fill_mask(H, W, poly)
        assert all(m[i, j] == zr.inside(poly, ref.centre(i, j)) for i in range(H) for j in range(W))
        assert m.any()
    # the vertex on a pixel centre
    assert polys[1][0] == ref.centre(8, 10)
    left, right = ref.fill_mask(H, W, polys[2]), ref.fill_mask(H, W, polys[3])
    union = ref.fill_mask(H, W, zr.quantise([(30.0, 5.0), (68.0, 5.0), (68.0, 30.0), (30.0, 30.0)]))
    assert not (left & right).any() and np.array_equal(left | right, union)
    # a shared edge through pixel centres (x = 40.5): every centre on it belongs to exactly one side
    a = ref.fill_mask(H, W, zr.quantise([(20.5, 4.0), (40.5, 4.0), (40.5, 30.0), (20.5, 30.0)]))
    b = ref.fill_mask(H, W, zr.quantise([(40.5, 4.0), (60.5, 4.0), (60.5, 30.0), (40.5, 30.0)]))
    whole = ref.fill_mask(H, W, zr.quantise([(20.5, 4.0), (60.5, 4.0), (60.5, 30.0), (20.5, 30.0)]))
    assert not (a & b).any() and np.array_equal(a | b, whole) and (a[:, 40] ^ b[:, 40]).sum() == whole[:, 40].sum() > 0


def test_tick_is_on_the_positive_side_in_all_eight_octants():
    from mydetection_amd import ops
    A = (333, -120)
    for t in (1, 2, 64):
        for dx, dy in ((400, 0), (400, 150), (150, 400), (0, 400), (-150, 400), (-400, 150), (-400, 0), (-400, -150), (-150, -400), (0, -400),
                       (150, -400), (400, -150), (1, 0), (0, -1)):
            line = (A, (A[0] + dx, A[1] + dy))
            m, e = ref.tick(line, t)
            assert m == ((2 * A[0] + dx) >> 1, (2 * A[1] + dy) >> 1)
            assert zr.side(line, e) > 0, (line, t, e)
            length2 = (e[0] - m[0]) ** 2 + (e[1] - m[1]) ** 2
            lh = math.isqrt(dx * dx + dy * dy)                           # 4 * thickness pixels: at most by Lh's floor longer, each
            assert (64 * t - 2) ** 2 <= length2 and length2 * lh * lh <= (64 * t) ** 2 * (dx * dx + dy * dy)     # coordinate truncated toward zero
            assert ops.overlay_tick(line[0] + line[1], t) == m + e
    assert ref.tick(((0, 0), (800, 800)), 2) == ((400, 400), (310, 490))   # n = (-800, 800), Lh = 1131: trunc(102400 / 1131) = 90
    assert ref.tick(((0, 0), (-3, 0)), 1) == ((-2, 0), (-2, -64))          # the midpoint floors


def test_label_texts():
    from mydetection_amd import ops
    all3 = ('occupancy', 'entries', 'visits')
    for v, shown in ((0, '0'), (9, '9'), (10, '10'), (999999, '999999'), (1000000, '999999')):
        assert ref.zone_text('z', all3, v, v, v) == f'z {shown} +{shown} -{shown}'
        assert ref.line_text('door', v, v) == f'door +{shown} -{shown}'
        assert ops.overlay_label_text('z', all3, v, v, v) == ref.zone_text('z', all3, v, v, v)
        assert ops.overlay_label_text('door', line=(v, v)) == ref.line_text('door', v, v)
    assert ref.zone_text('hall', ('entries',), 5, 6, 7) == 'hall +6' and ref.zone_text('hall', (), 5, 6, 7) == 'hall'
    assert ops.overlay_label_text('hall', ('visits', 'occupancy'), 5, 6, 7) == 'hall 5 -7'          # the order is the rule's, not the caller's
    assert ref.zone_text('', ('occupancy',), 3, 0, 0) == ' 3'
    long = 'a-name-longer-than-sixteen'
    worst = ref.zone_text(long, all3, 10 ** 7, 10 ** 7, 10 ** 7)
    assert worst == 'a-name-longer-th 999999 +999999 -999999' and len(worst) == 39 <= ref.MAX_GLYPHS
    assert ops.overlay_label_text(long, all3, 10 ** 7, 10 ** 7, 10 ** 7) == worst
    # the 40-glyph cut: no text of the rule is longer, and the cut holds for any text
    assert len(ref.line_text(long, 10 ** 7, 10 ** 7)) == 32
    assert ('x' * 50)[:ref.MAX_GLYPHS] == 'x' * 40 and ops._lib.OVERLAY_MAX_GLYPHS == ref.MAX_GLYPHS == 40
    # the rectangle: the renderer's clamps at an anchor
    assert ref.label_rect(37, 70, (16 * 50, 16 * 5), 13, 8, 5) == (5, 0)       # clamped at the right (70 - 65) and at the top
    assert ref.label_rect(37, 70, (16 * 10 + 15, 16 * 20 + 15), 3, 8, 5) == (10, 12)
    assert ref.label_rect(37, 70, (-40, 16 * 100), 20, 8, 5) == (0, 29)        # wider than the frame: left 0; below: the last rows


def test_geometry_of_a_zone_set():
    from mydetection_amd import _lib, ops
    zs = ops.zone_set((37, 70), oc.POLYGONS, oc.LINES)
    g = ops.overlay_geometry(zs, oc.NAMES, 2)
    assert (g.n_polygons, g.n_lines, g.thickness) == (5, 2, 2)
    for z, poly in enumerate(oc.POLYGONS):
        q = zr.quantise(poly)
        assert [tuple(g.struct.polygon[z][i]) for i in range(g.struct.n_vertices[z])] == q
        assert tuple(g.struct.anchor[z]) == min(q, key=lambda p: (p[1], p[0]))
    for l, line in enumerate(oc.LINES):
        q = tuple(zr.quantise(line))
        m, e = ref.tick(q, 2)
        assert tuple(g.struct.line[l]) == q[0] + q[1] and tuple(g.struct.tick[l]) == m + e and tuple(g.struct.anchor[16 + l]) == m
    assert bytes(g.struct.name[1]) == b'a-name-longer-th' and bytes(g.struct.name[0]) == b'hall' + bytes(12)
    assert bytes(g.struct.name[16]) == b'door' + bytes(12) and bytes(g.struct.name[4]) == bytes(16)
    assert len(bytes(g.struct)) == 3392
    with pytest.raises(TypeError, match='ZoneSet'):
        ops.overlay_geometry('zones')
    with pytest.raises(ValueError, match='names'):
        ops.overlay_geometry(zs, ['a'])
    for t in (0, 65, 2.0, True):
        with pytest.raises(ValueError, match='thickness'):
            ops.overlay_geometry(zs, None, t)
    assert _lib.TRAIL_MAX_POINTS == 32


# ------------------------------------------------------------------------------------------------------------------- trails
def _frame(stream, rows, count=0):
    """rows: slot -> (id, x, y, cls, missed); the other slots free."""
    mt = stream.mt
    box, ids, cls, missed = np.zeros((mt, 5), np.float32), [0] * mt, [0] * mt, [-1] * mt
    for t, (tid, x, y, c, ms) in rows.items():
        box[t, :4] = (x, y, 4, 6)
        ids[t], cls[t], missed[t] = tid, c, ms
    return stream.frame(box, ids, cls, missed, count)


def test_trails_ring_by_hand():
    st = ref.TrailStream(2, 3)
    for f in range(5):                                                   # ring wrap: F = 5 > L = 3
        pts, lens, bbox = _frame(st, {0: (7, float(f), 2.0 * f, 0, 0)})
    assert pts[0] == [[64, 128], [48, 96], [32, 64]] and lens == [3, 0] and bbox[0] == [32, 64, 64, 128] and bbox[1] == [0, 0, 0, 0]
    assert st.head[0] == 2 and st.fill[0] == 3 and st.arrays()['ring'][0].tolist() == [[48, 96], [64, 128], [32, 64]]
    pts, lens, _ = _frame(st, {0: (7, 9.0, 9.0, 0, 2)})                # coasting: nothing pushed, the trail stands
    assert pts[0][0] == [64, 128] and lens[0] == 3
    pts, lens, _ = _frame(st, {0: (7, 9.0, 9.0, 0, 0)}, count=-1)      # a bad-class frame: the state stands, the outputs come from it
    assert pts[0][0] == [64, 128] and lens[0] == 3 and st.fill[0] == 3
    pts, lens, _ = _frame(st, {}, count=-1)                              # ... and len is 0 where the tracker's id differs
    assert lens[0] == 0 and st.id[0] == 7
    pts, lens, bbox = _frame(st, {0: (8, 1.0, 1.0, 0, 0)})              # slot reuse with a new id: cleared, then one point
    assert st.id[0] == 8 and pts[0] == [[16, 16], [0, 0], [0, 0]] and lens[0] == 1 and st.head[0] == 1 and bbox[0] == [16, 16, 16, 16]
    pts, lens, _ = _frame(st, {0: (8, float('nan'), 1.0, 0, 0), 1: (9, 1.0, float('inf'), 0, 0)})     # non-finite: unobserved
    assert lens == [1, 0] and st.id[1] == 0
    pts, lens, _ = _frame(st, {})                                        # the track is gone: cleared
    assert st.id[0] == 0 and st.fill[0] == 0 and st.arrays()['ring'].sum() == 0 and lens == [0, 0]
    flt = ref.TrailStream(2, 2, classes=[3])                             # the class filter
    _, lens, _ = _frame(flt, {0: (5, 1.0, 1.0, 3, 0), 1: (6, 1.0, 1.0, 2, 0)})
    assert lens == [1, 0] and flt.id == [5, 0]
    bot = ref.TrailStream(1, 2, anchor='bottom')
    pts, _, _ = _frame(bot, {0: (5, 1.0, 1.0, 0, 0)})
    assert pts[0][0] == [16, 64]                                         # cy + h / 2 = 4


@pytest.mark.parametrize('name', ['fuzz_L7', 'reuse_L2', 'bad_frame', 'mt1'])
def test_trails_split_calls_equal_one_call(name):
    case = oc.trail_cases()[name]
    S, F, MT = case['out']['id'].shape
    ts = case['ts']

    def streams():
        return [ref.TrailStream(MT, ts['max_points'], ts.get('anchor', 'center'), ts.get('classes')) for _ in range(S)]
    one = streams()
    want = ref.run_trails(one, case['out'])
    two = streams()
    cut = F // 3
    parts = [ref.run_trails(two, {k: v[:, lo:hi] for k, v in case['out'].items()}) for lo, hi in ((0, cut), (cut, F))]
    for k in want:
        assert np.array_equal(np.concatenate([p[k] for p in parts], axis=1), want[k]), k
    for a, b in zip(one, two):
        assert all(np.array_equal(a.arrays()[k], b.arrays()[k]) for k in a.arrays())
    assert want['len'].max() == min(ts['max_points'], want['len'].max()) and want['len'].max() >= 2


def test_paint_order_and_chroma_rule_of_the_restatement():
    """Two crossing strokes and a label on a 6 x 8 frame, by hand: the later operation wins a pixel; a chroma sample takes every
    operation that touches its quad, the last one staying."""
    H, W = 6, 8
    red, green = np.array([255, 0, 0], np.uint8), np.array([0, 255, 0], np.uint8)
    m1, m2 = ref.capsule_mask(H, W, (8, 40), (120, 40), 1), ref.capsule_mask(H, W, (56, 8), (56, 88), 1)
    assert m1.sum() == 8 and m1[2].all() and m2.sum() == 6 and m2[:, 3].all()
    img = np.zeros((H, W, 3), np.uint8)
    ref.paint_rgb(img, [('blend', np.ones((H, W), bool), red, 51), ('set', m1, red), ('set', m2, green)])
    assert img[2, 3].tolist() == [0, 255, 0] and img[2, 0].tolist() == [255, 0, 0] and img[0, 0].tolist() == [51, 0, 0]
    Y, U, V = np.full((H, W), 100, np.uint8), np.full((3, 4), 128, np.uint8), np.full((3, 4), 128, np.uint8)
    ref.paint_yuv(Y, U, V, [('set', m1, red), ('set', m2, green)])
    from mydetection_amd import ops
    ry, ru, rv = (int(v) for v in ops.rgb_to_yuv(red))
    gy, gu, gv = (int(v) for v in ops.rgb_to_yuv(green))
    assert Y[2, 0] == ry and Y[2, 3] == gy and Y[3, 0] == 100
    assert (U[1, 0], V[1, 0]) == (ru, rv) and (U[1, 1], V[1, 1]) == (gu, gv) and (U[0, 1], V[0, 1]) == (gu, gv) and (U[0, 0], V[0, 0]) == (128, 128)


# ------------------------------------------------------------------------------------------------------------ argument rules
def test_overlay_settings_are_checked_without_a_device():
    from mydetection_amd.api import Overlay, Tracker, Zones
    Overlay()
    Overlay(zones=False, lines=False, trails=2, counters=())
    with pytest.raises(ValueError, match='nothing to paint'):
        Overlay(zones=False, lines=False, trails=0)
    for bad in (1, 33, -1, 2.0, True):
        with pytest.raises(ValueError, match='trails'):
            Overlay(trails=bad)
    for kw in (dict(zone_alpha=256), dict(occupied_alpha=-1), dict(zone_alpha=1.5)):
        with pytest.raises(ValueError, match='alpha'):
            Overlay(**kw)
    with pytest.raises(ValueError, match='counter'):
        Overlay(counters=('exits',))
    for kw in (dict(thickness=0), dict(trail_thickness=65)):
        with pytest.raises(ValueError, match='thickness'):
            Overlay(**kw)
    with pytest.raises(ValueError, match='label_height'):
        Overlay(label_height=7)
    with pytest.raises(ValueError, match='classes'):
        Overlay(classes=[-1])
    ov = Overlay(trails=4)
    assert ov.sizes((1080, 1920)) == (3, 3, 24) and ov.sizes((150, 200))[:2] == (1, 1)
    trk, zones = Tracker(), Zones(polygons=[[(0, 0), (9, 0), (9, 9)]])
    with pytest.raises(ValueError, match='tracker='):
        ov.check_call(None, zones, (10, 10))
    with pytest.raises(ValueError, match='zones='):
        ov.check_call(trk, None, (10, 10))
    with pytest.raises(ValueError, match='nothing to paint'):
        Overlay(zones=False, lines=True).check_call(trk, zones, (10, 10))
    ov.check_call(trk, zones, (10, 10))
    Overlay(zones=False, lines=False, trails=2).check_call(trk, None, (10, 10))
    assert ov.state is None and ov.img_hw is None


def test_ops_argument_rules_touch_no_device():
    from mydetection_amd import ops
    for bad in (1, 33, 2.5, True):
        with pytest.raises(ValueError, match='max_points'):
            ops.trail_set(bad)
    with pytest.raises(ValueError, match='anchor'):
        ops.trail_set(2, 'top')
    with pytest.raises(ValueError, match='classes'):
        ops.trail_set(2, classes=list(range(17)))
    ts = ops.trail_set(5, 'bottom', [3, 4])
    assert (ts.max_points, ts.anchor, ts.n_classes, list(ts.classes[:2])) == (5, 1, 2, [3, 4])
    assert ops.trails_state_words(3, 2) == 24 and ops.trails_state_words(512, 32) == 512 * 68 and ops.trails_state_words(1, 2) == 8
    for mt, L in ((0, 2), (513, 2), (4, 1), (4, 33)):
        with pytest.raises(ValueError):
            ops.trails_state_words(mt, L)
    state = torch.zeros((2, 24), dtype=torch.int32)
    v = ops.trails_state_views(state, 3, 2)
    assert {k: tuple(t.shape) for k, t in v.items()} == {'id': (2, 3), 'fill': (2, 3), 'head': (2, 3), 'ring': (2, 3, 2, 2)}
    with pytest.raises(ValueError, match='words'):
        ops.trails_state_views(state, 4, 2)
    S, F, MT = 1, 2, 3
    out = {'box': torch.zeros((S, F, MT, 5)), 'id': torch.zeros((S, F, MT), dtype=torch.int64), 'cls': torch.zeros((S, F, MT), dtype=torch.int64),
           'missed': torch.zeros((S, F, MT), dtype=torch.int32), 'count': torch.zeros((S, F), dtype=torch.int32)}
    with pytest.raises(TypeError, match='TrailSet'):
        ops.trails_frames(out, state, 'trails')
    with pytest.raises(ValueError, match='state'):
        ops.trails_frames(out, torch.zeros((1, 20), dtype=torch.int32), ops.trail_set(2))
    with pytest.raises(ValueError, match="'missed'"):
        ops.trails_frames(dict(out, missed=out['missed'].long()), state[:1], ops.trail_set(2))
    # draw_overlay: every rule before the device check (CPU tensors are refused last)
    frames = torch.zeros((2, 8, 8, 3), dtype=torch.uint8)
    style = ops.draw_style()
    zs = ops.zone_set((8, 8), [[(0, 0), (7, 0), (7, 7)]], [((0, 0), (5, 5))])
    geo = ops.overlay_geometry(zs)
    zout = {'occupancy': torch.zeros((1, 2, 1), dtype=torch.int32), 'zone_counts': torch.zeros((1, 2, 1, 4), dtype=torch.int32),
            'line_counts': torch.zeros((1, 2, 1, 2), dtype=torch.int32)}
    tout = {'points': torch.zeros((1, 2, 3, 4, 2), dtype=torch.int32), 'len': torch.zeros((1, 2, 3), dtype=torch.int32),
            'bbox': torch.zeros((1, 2, 3, 4), dtype=torch.int32)}
    trk = {'id': torch.zeros((1, 2, 3), dtype=torch.int64), 'missed': torch.zeros((1, 2, 3), dtype=torch.int32)}
    with pytest.raises(TypeError, match='style'):
        ops.draw_overlay(frames, None, geometry=geo, zones_out=zout)
    with pytest.raises(ValueError, match='nothing to paint'):
        ops.draw_overlay(frames, style)
    with pytest.raises(ValueError, match='nothing to paint'):
        ops.draw_overlay(frames, style, geometry=geo, zones_out=zout, zones=False, lines=False)
    with pytest.raises(TypeError, match='OverlayGeometry'):
        ops.draw_overlay(frames, style, geometry=zs, zones_out=zout)
    with pytest.raises(ValueError, match='zones_out'):
        ops.draw_overlay(frames, style, geometry=geo)
    with pytest.raises(ValueError, match='zone_counts'):
        ops.draw_overlay(frames, style, geometry=geo, zones_out=dict(zout, zone_counts=zout['zone_counts'][..., :3]))
    with pytest.raises(ValueError, match='counter'):
        ops.draw_overlay(frames, style, geometry=geo, zones_out=zout, counters=('dwell',))
    for kw in (dict(zone_alpha=300), dict(occupied_alpha=-2), dict(trail_thickness=0)):
        with pytest.raises(ValueError, match='alpha|thickness'):
            ops.draw_overlay(frames, style, geometry=geo, zones_out=zout, **kw)
    with pytest.raises(ValueError, match='track_out'):
        ops.draw_overlay(frames, style, trails_out=tout)
    with pytest.raises(ValueError, match="'missed'"):
        ops.draw_overlay(frames, style, trails_out=tout, track_out=dict(trk, missed=trk['missed'][:, :1]))
    with pytest.raises(ValueError, match='frames'):
        ops.draw_overlay(frames[:1], style, geometry=geo, zones_out=zout)
    with pytest.raises(ValueError, match='1 x 2'):
        ops.draw_overlay(frames, style, geometry=geo, zones_out=zout, trails_out={k: v[:, :1] for k, v in tout.items()},
                         track_out={k: v[:, :1] for k, v in trk.items()})
    with pytest.raises(TypeError, match='uint8'):
        ops.draw_overlay(frames.float(), style, geometry=geo, zones_out=zout)
    with pytest.raises(ValueError, match='p010'):
        ops.draw_overlay_yuv420((torch.zeros((2, 8, 8), dtype=torch.int16), torch.zeros((2, 4, 4, 2), dtype=torch.int16)), 'p010', style,
                                geometry=geo, zones_out=zout)
    with pytest.raises(Exception, match='no CPU path'):                  # everything is in order but the device: refused, nothing launched
        ops.draw_overlay(frames, style, geometry=geo, zones_out=zout, trails_out=tout, track_out=trk)
    assert int(frames.sum()) == 0


def test_header_declares_the_entry_points_and_constants():
    from mydetection_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'mydet.h')).read()
    for name in ('mydet_trails_state_words', 'mydet_trails_reset', 'mydet_trails_frames', 'mydet_draw_overlay_rgb_u8', 'mydet_draw_overlay_yuv420_u8'):
        assert re.search(r'\b(?:int|int64_t)\s+' + name + r'\s*\(', header) and name in _lib.SIGNATURES, name
    consts = {m.group(1): int(m.group(2)) for m in re.finditer(r'#define MYDET_(OVERLAY_\w+|TRAIL_\w+)\s+(\d+)', header)}
    assert consts == {'OVERLAY_MAX_GLYPHS': _lib.OVERLAY_MAX_GLYPHS, 'OVERLAY_ZONES': _lib.OVERLAY_ZONES, 'OVERLAY_LINES': _lib.OVERLAY_LINES,
                      'OVERLAY_TRAILS': _lib.OVERLAY_TRAILS, 'OVERLAY_COUNT_OCCUPANCY': _lib.OVERLAY_COUNT_OCCUPANCY,
                      'OVERLAY_COUNT_ENTRIES': _lib.OVERLAY_COUNT_ENTRIES, 'OVERLAY_COUNT_VISITS': _lib.OVERLAY_COUNT_VISITS,
                      'TRAIL_MAX_POINTS': _lib.TRAIL_MAX_POINTS}
    assert f'#define MYDET_ABI_VERSION {_lib.ABI_VERSION} ' in header and _lib.ABI_VERSION == 2


def test_scenes_restate_to_something():
    """The scenes the GPU tests use paint what their names say (the restatement alone, small and quick)."""
    hw = oc.RGB_HW
    sc = oc.scenes(*hw)
    assert all(not op[1].any() for op in ref.frame_ops(sc['nothing'], 0, *hw))
    ops0, ops1 = ref.frame_ops(sc['zones_t1'], 0, *hw), ref.frame_ops(sc['zones_t1'], 1, *hw)
    assert [op[3] for op in ops0 if op[0] == 'blend'] == [48] * 5 and [op[3] for op in ops1 if op[0] == 'blend'] == [96, 48, 96, 48, 96]
    assert sum(op[0] == 'label' for op in ops0) == 7 and sum(op[0] == 'set' for op in ops0) == 4 + 3 + 4 + 4 + 3 + 4
    lab = [op for op in ops0 if op[0] == 'label'][3]                     # 'right': clamped at the right edge and at the top
    rows, cols = np.nonzero(lab[1])
    assert rows.min() == 0 and cols.max() == hw[1] - 1
    tr = sc['trails32_mt64']['trails']
    assert tr['len'].max() == 32 and (tr['missed'] > 0).any() and (tr['len'][tr['missed'] > 0] >= 2).any()
