"""CPU tests of zone and line counting (include/mydet.h: mydet_zones_frames): the header, the ctypes table and the library
agree; every ValueError of ops.zone_set and api.Zones is raised without a device; the quantisation; and the restatement
tests/_zones_ref.py -- the checker of tests/test_gpu_zones.py -- against exact fractions, on hand cases and across calls."""
import ctypes
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

import _zones_cases as zc
import _zones_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_table_library_and_constants_agree():
    from mydetection_amd import _lib, ops
    header = open(os.path.join(ROOT, 'include', 'mydet.h')).read()
    defs = {m.group(1): int(m.group(2)) for m in re.finditer(r'#define MYDET_(ZONES?_\w+)\s+(\d+)', header)}
    want = {'ZONES_MAX': _lib.ZONES_MAX, 'ZONE_MAX_VERTICES': _lib.ZONE_MAX_VERTICES, 'ZONE_MAX_CLASSES': _lib.ZONE_MAX_CLASSES,
            'ZONE_MAX_HEAT': _lib.ZONE_MAX_HEAT, 'ZONE_MAX_FRAME': _lib.ZONE_MAX_FRAME, 'ZONE_COORD_MAX': _lib.ZONE_COORD_MAX,
            'ZONE_ANCHOR_CENTER': _lib.ZONE_ANCHOR_CENTER, 'ZONE_ANCHOR_BOTTOM': _lib.ZONE_ANCHOR_BOTTOM,
            'ZONES_STATE_HEADER': _lib.ZONES_STATE_HEADER, 'ZONES_SLOT_WORDS': _lib.ZONES_SLOT_WORDS}
    assert defs == want
    assert (ref.ZMAX, ref.COORD_MAX, ref.BAD_CLASS) == (_lib.ZONES_MAX, _lib.ZONE_COORD_MAX, -1) and '#define MYDET_COUNT_BAD_CLASS (-1)' in header
    # the struct: every field an int, in the header's order
    body = re.search(r'typedef struct mydet_zone_set \{(.*?)\} mydet_zone_set;', header, re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    names = [n for decl in body.split(';') if decl.strip() for n in re.findall(r'(\w+)(?:\[[\w\]\[]+)?\s*(?:,|$)', decl.strip()[len('int'):])]
    assert names == [f[0] for f in _lib.ZoneSet._fields_]
    assert ctypes.sizeof(_lib.ZoneSet) == 4 * (12 + 16 + 16 * 16 * 2 + 16 * 4 + 16)
    assert _lib.ABI_VERSION == 2
    lib = _lib.lib()
    for name in ('mydet_zones_state_words', 'mydet_zones_reset', 'mydet_zones_frames'):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    for mt in (1, 2, 64, 65, 511, 512):
        assert lib.mydet_zones_state_words(mt) == ops.zones_state_words(mt) and ops.zones_state_words(mt) % 4 == 0
        assert ops.zones_state_words(mt) >= _lib.ZONES_STATE_HEADER + _lib.ZONES_SLOT_WORDS * mt
    assert lib.mydet_zones_state_words(0) == 0 and lib.mydet_zones_state_words(513) == 0
    for bad in (0, 513):
        with pytest.raises(ValueError):
            ops.zones_state_words(bad)


def test_the_c_entry_points_refuse_bad_arguments_before_any_launch():
    from mydetection_amd import _lib, ops
    lib = _lib.lib()
    null, p = ctypes.c_void_p(0), ctypes.c_void_p(4096)              # never dereferenced: every call below returns before a launch
    assert lib.mydet_zones_reset(null, 1, 8, null) == -1 and lib.mydet_zones_reset(p, 0, 8, null) == -1
    assert lib.mydet_zones_reset(ctypes.c_void_p(4100), 1, 8, null) == -1 and lib.mydet_zones_reset(p, 1, 513, null) == -2
    zs = ops.zone_set((48, 64), polygons=[zc.SQUARE], lines=[zc.LINE], heat=(4, 8))

    def call(z=zs, S=1, F=1, mt=8, **ptrs):
        a = {k: p for k in ('box', 'id', 'cls', 'missed', 'count', 'state', 'heat', 'inside', 'crossed', 'dwell', 'occ', 'zc', 'lc')}
        a.update(ptrs)
        return lib.mydet_zones_frames(a['box'], a['id'], a['cls'], a['missed'], a['count'], S, F, mt, ctypes.byref(z), a['state'], a['heat'],
                                      a['inside'], a['crossed'], a['dwell'], a['occ'], a['zc'], a['lc'], null)

    assert call(mt=513) == -2
    assert call(S=0) == -1 and call(F=0) == -1 and call(mt=0) == -1
    for k in ('box', 'id', 'cls', 'missed', 'count', 'state', 'heat', 'inside', 'crossed', 'dwell', 'occ', 'zc', 'lc'):
        assert call(mt=513, **{k: null}) == -1, k
    assert call(mt=513, state=ctypes.c_void_p(4104)) == -1 and call(mt=513, id=ctypes.c_void_p(4100)) == -1

    def broken(**fields):
        z = _lib.ZoneSet.from_buffer_copy(zs)
        for k, v in fields.items():
            setattr(z, k, v)
        return z

    for fields in ({'n_polygons': 17}, {'n_lines': -1}, {'n_polygons': 0, 'n_lines': 0}, {'n_classes': 17}, {'anchor': 2}, {'coasting': 2},
                   {'img_h': 0}, {'img_w': 32769}, {'heat_h': 0}, {'heat_w': 1025}):
        assert call(z=broken(**fields), mt=513) == -1, fields
    z = broken()
    z.n_vertices[0] = 2
    assert call(z=z, mt=513) == -1
    z = broken()
    z.polygon[0][1][0] = (1 << 20) + 1
    assert call(z=z, mt=513) == -1
    z = broken()
    for i in range(4):
        z.polygon[0][i][1] = 0                                       # no area
    assert call(z=z, mt=513) == -1
    z = broken()
    z.line[0][:] = [5, 5, 5, 5]
    assert call(z=z, mt=513) == -1
    # without polygons the three zone outputs may be null, without lines the line output, without a heat grid the heat map
    lines_only = ops.zone_set((48, 64), lines=[zc.LINE])
    assert call(z=lines_only, mt=513, dwell=null, occ=null, zc=null, heat=null) == -2
    assert call(z=ops.zone_set((48, 64), polygons=[zc.SQUARE]), mt=513, lc=null, heat=null) == -2


def test_quantisation_at_sixteenths_and_just_below():
    from mydetection_amd import ops
    for k in (-33, -16, -1, 0, 1, 15, 16, 17, 1000, 16 * 4096 + 7):
        v = np.float32(k) / np.float32(16)
        below = np.nextafter(v, np.float32(-np.inf), dtype=np.float32)
        assert ref.q(v) == k and ref.q(below) == k - 1
        assert ops.zone_quantise([v, below]).tolist() == [k, k - 1]
    big = [1e9, -1e9, 65536.0, -65536.0, 65535.99, 3e38, -3e38]
    want = [1 << 20, -(1 << 20), 1 << 20, -(1 << 20), 1048575, 1 << 20, -(1 << 20)]
    with np.errstate(over='ignore'):
        assert ops.zone_quantise(big).tolist() == want and [ref.q(v) for v in big] == want
    zs = ops.zone_set((48, 64), polygons=[[(0.06, 0.07), (20, 0), (20.99, 20.5)]], lines=[((1, 2), (3.5, 4.25))])
    assert [list(zs.polygon[0][i]) for i in range(3)] == [[0, 1], [320, 0], [335, 328]] and zs.n_vertices[0] == 3
    assert list(zs.line[0]) == [16, 32, 56, 68]
    r = ref.ZoneSet((48, 64), polygons=[[(0.06, 0.07), (20, 0), (20.99, 20.5)]], lines=[((1, 2), (3.5, 4.25))])
    assert r.polygons == [[(0, 1), (320, 0), (335, 328)]] and r.lines == [((16, 32), (56, 68))]


def test_zone_set_raises_for_everything_out_of_range():
    from mydetection_amd import ops
    sq, ln = zc.SQUARE, zc.LINE
    nan, inf = float('nan'), float('inf')
    bad = [dict(), dict(polygons=[], lines=[]),                                                # neither polygons nor lines
           dict(polygons=[sq] * 17), dict(lines=[ln] * 17),
           dict(polygons=[sq[:2]]), dict(polygons=[[(i, i * i) for i in range(17)]]),          # 2 and 17 vertices
           dict(polygons=[[(0, 0), (10, 10), (20, 20)]]),                                      # no area
           dict(polygons=[[(0, 0), (0.01, 0), (0, 0.01)]]),                                    # no area once quantised
           dict(polygons=[[(0, 0), (10, 0), (10, 10), (0, 0), (-10, -10), (-10, 0)]]),         # two lobes that cancel
           dict(lines=[((5, 5), (5, 5))]), dict(lines=[((5, 5), (5.01, 5.01))]),               # no length (once quantised)
           dict(polygons=[[(0, 0), (nan, 0), (0, 10)]]), dict(polygons=[[(0, 0), (inf, 0), (0, 10)]]), dict(lines=[((0, 0), (0, -inf))]),
           dict(lines=[((0, 0), (1e39, 0))]),
           dict(polygons=[[(0, 0, 0), (1, 1, 1), (2, 0, 2)]]), dict(polygons=[5]), dict(lines=[(0, 0, 5, 5)]), dict(lines=[((0, 0),)]),
           dict(lines=[ln], anchor='top'), dict(lines=[ln], anchor=None),
           dict(lines=[ln], classes=[]), dict(lines=[ln], classes=list(range(17))), dict(lines=[ln], classes=[-1]),
           dict(lines=[ln], heat=(0, 8)), dict(lines=[ln], heat=(8, 1025)), dict(lines=[ln], heat=8), dict(lines=[ln], heat=(4, 4, 4))]
    for kw in bad:
        with pytest.raises(ValueError):
            ops.zone_set((48, 64), **kw)
    for hw in ((0, 64), (48, 32769), (48,), None):
        with pytest.raises(ValueError):
            ops.zone_set(hw, lines=[ln])
    zs = ops.zone_set((32768, 32768), polygons=[sq] * 16, lines=[ln] * 16, anchor='bottom', classes=range(16), coasting=1, heat=(1024, 1))
    assert (zs.n_polygons, zs.n_lines, zs.n_classes, zs.anchor, zs.coasting, zs.heat_h, zs.heat_w) == (16, 16, 16, 1, 1, 1024, 1)
    assert list(zs.classes) == list(range(16)) and (zs.img_h, zs.img_w) == (32768, 32768)
    with pytest.raises(TypeError):
        ops.zones_frames({'box': torch.zeros(1, 1, 1, 5)}, None, 'zones')
    with pytest.raises(ValueError):
        ops.zones_heat(1, ops.zone_set((48, 64), lines=[ln]), 'cpu')


def test_zones_object_raises_without_a_device():
    from mydetection_amd.api import Detector, Tracker, Zones
    sq, ln = zc.SQUARE, zc.LINE
    for kw in (dict(), dict(polygons=[sq[:2]]), dict(lines=[((1, 1), (1, 1))]), dict(lines=[ln], anchor='left'), dict(lines=[ln], heat=(0, 0)),
               dict(lines=[ln], classes=[]), dict(polygons=5), dict(polygons=[sq], lines=[ln], names=['a']), dict(polygons=[[(0, float('nan')), (1, 1), (2, 0)]])):
        with pytest.raises(ValueError):
            Zones(**kw)
    z = Zones(polygons=[sq], lines=[ln], names=['door', 'gate'], heat=(4, 8))
    assert z.names == ['door', 'gate'] and z.state is None and z.last is None and z.heat is None and z.counts() == []
    assert Zones(polygons=[sq], lines=[ln]).names == ['zone0', 'line0']
    z.reset()                                                        # before the first call: nothing to do
    # zones= needs tracker=, and a Zones
    with pytest.raises(ValueError, match='tracker='):
        Detector._pop_zones({'zones': z}, None)
    with pytest.raises(TypeError):
        Detector._pop_zones({'zones': object()}, Tracker())
    kwargs = {'zones': z, 'conf_thres': 0.3}
    assert Detector._pop_zones(kwargs, Tracker()) is z and kwargs == {'conf_thres': 0.3} and Detector._pop_zones({}, None) is None
    with pytest.raises(TypeError):
        Detector._no_tracker({'zones': z}, 'frames_to_json')
    # the box format and the frame size, before any launch
    zb = Zones(polygons=[sq], anchor='bottom')
    with pytest.raises(ValueError, match='bottom'):
        zb.check_call(Tracker(), (48, 64), 'cxcywhd')
    zb.check_call(Tracker(), (48, 64), 'cxcywh')
    with pytest.raises(ValueError):
        z.check_call(Tracker(), (48, 40000), 'cxcywh')
    # a bound object refuses another tracker shape or frame size
    z.streams, z.max_tracks, z.img_hw = 2, 64, (48, 64)
    z.check_call(Tracker(streams=2, max_tracks=64), (48, 64), 'cxcywh')
    for trk, hw in ((Tracker(streams=1, max_tracks=64), (48, 64)), (Tracker(streams=2, max_tracks=65), (48, 64)),
                    (Tracker(streams=2, max_tracks=64), (64, 48))):
        with pytest.raises(ValueError, match='bound to'):
            z.check_call(trk, hw, 'cxcywh')


# ---- the restatement's geometry against exact fractions ----

def exact_inside(poly, p):
    """The crossing number with the half-open rule, in rational arithmetic: an edge whose ends straddle p's row (one end strictly
    above, by y > p.y) counts when it meets the row strictly to the right of p."""
    n, hit = len(poly), False
    for i in range(n):
        (ax, ay), (bx, by) = poly[i], poly[(i + 1) % n]
        if (ay > p[1]) != (by > p[1]):
            x_at = Fraction(ax) + Fraction(p[1] - ay) * Fraction(bx - ax, by - ay)
            if Fraction(p[0]) < x_at:
                hit = not hit
    return hit


def test_inside_rule_on_hand_cases():
    sq = [(0, 0), (8, 0), (8, 8), (0, 8)]
    # a vertex: the corner of least x and y is inside, the other three are not; a horizontal edge: the one of least y is inside
    assert [ref.inside(sq, v) for v in sq] == [True, False, False, False]
    assert ref.inside(sq, (3, 0)) and not ref.inside(sq, (3, 8)) and ref.inside(sq, (0, 3)) and not ref.inside(sq, (8, 3))
    assert ref.inside(sq, (4, 4)) and not ref.inside(sq, (9, 4)) and not ref.inside(sq, (-1, 4)) and not ref.inside(sq, (4, -1))
    assert ref.inside(sq[::-1], (4, 4)) and [ref.inside(sq[::-1], v) for v in sq] == [True, False, False, False]      # either orientation
    # a shared edge of two polygons: every point of it is inside exactly one of them
    left, right = [(0, 0), (8, 0), (8, 8), (0, 8)], [(8, 0), (16, 0), (16, 8), (8, 8)]
    for y in range(0, 8):
        assert ref.inside(left, (8, y)) + ref.inside(right, (8, y)) == 1
    lower, upper = [(0, 0), (8, 0), (8, 8)], [(0, 0), (8, 8), (0, 8)]
    for k in range(0, 8):
        assert ref.inside(lower, (k, k)) + ref.inside(upper, (k, k)) == 1
    # a concave polygon: the notch is outside, its tip's neighbourhood decides by the rule
    arrow = [(0, 0), (16, 0), (16, 12), (8, 4), (0, 12)]
    assert ref.inside(arrow, (8, 3)) and not ref.inside(arrow, (8, 5)) and ref.inside(arrow, (2, 9)) and ref.inside(arrow, (14, 9))
    assert not ref.inside(arrow, (8, 11)) and ref.inside(arrow, (8, 4)) == exact_inside(arrow, (8, 4))
    for p in [(x, y) for x in range(-1, 18) for y in range(-1, 14)]:
        assert ref.inside(arrow, p) == exact_inside(arrow, p), p


def test_inside_rule_on_a_lattice_against_exact_fractions():
    rng = np.random.RandomState(7)
    checked = on_edge = 0
    for trial in range(60):
        n = int(rng.randint(3, 9))
        poly = [(int(x), int(y)) for x, y in rng.randint(-6, 7, (n, 2))]          # self-intersecting ones included: even-odd is defined
        for x in range(-7, 8):
            for y in range(-7, 8):
                assert ref.inside(poly, (x, y)) == exact_inside(poly, (x, y)), (poly, x, y)
                checked += 1
                on_edge += any(ref.cross(ref.sub(poly[(i + 1) % n], poly[i]), ref.sub((x, y), poly[i])) == 0 for i in range(n))
    assert checked == 60 * 225 and on_edge > 1000
    # a partition: each lattice point of the whole is in exactly one part, each point outside the whole in none
    whole = [(-6, -6), (6, -6), (6, 6), (-6, 6)]
    for _ in range(40):
        c = (int(rng.randint(-5, 6)), int(rng.randint(-5, 6)))
        parts = [[whole[i], whole[(i + 1) % 4], c] for i in range(4)]            # four triangles around an inner point
        for x in range(-7, 8):
            for y in range(-7, 8):
                assert sum(ref.inside(t, (x, y)) for t in parts) == ref.inside(whole, (x, y)), (c, x, y)
    # the same far from the origin, where the products need more than 32 bits
    big = [(-(1 << 20), -(1 << 20)), ((1 << 20), -(1 << 20) + 3), ((1 << 20) - 5, (1 << 20)), (-(1 << 20) + 1, (1 << 20) - 7)]
    for p in [(0, 0), ((1 << 20), 0), ((1 << 20) - 3, 17), (-(1 << 20), -(1 << 20)), (12345, (1 << 20) - 1), (-(1 << 20) + 1, 999999)]:
        assert ref.inside(big, p) == exact_inside(big, p)


def test_side_and_segment_rules():
    line = ((0, 0), (0, 10))                                         # towards +y: x < 0 is positive
    assert [ref.side(line, p) for p in ((-1, 5), (1, 5), (0, 5), (0, 50), (-3, -9))] == [1, -1, 0, 0, 1]
    assert ref.segment_test(line, (-2, 5), (2, 5)) and ref.segment_test(line, (-2, 0), (2, 0)) and ref.segment_test(line, (-2, 10), (2, 10))
    assert not ref.segment_test(line, (-2, 11), (2, 11)) and not ref.segment_test(line, (-2, -1), (2, -1))
    assert ref.segment_test(line, (-2, 8), (2, 12)) and not ref.segment_test(line, (-2, 9), (2, 13))      # through B; just past it
    assert ref.segment_test(line, (0, 5), (3, 5)) and not ref.segment_test(line, (0, 12), (3, 12))       # starting on the line


# ---- the restatement as a whole ----

def _run_ref(case, splits=None):
    out = case['out']
    S, F, MT = out['id'].shape
    zs = ref.ZoneSet(case['img_hw'], **case['zs'])
    streams = [ref.Stream(MT) for _ in range(S)]
    heat = None if zs.heat is None else np.zeros((S,) + tuple(zs.heat), np.int64)
    parts, lo = [], 0
    for n in splits or [F]:
        parts.append(ref.run(zs, streams, {k: v[:, lo:lo + n] for k, v in out.items()}, heat))
        lo += n
    assert lo == F
    return {k: np.concatenate([p[k] for p in parts], axis=1) for k in parts[0]}, streams, heat


@pytest.mark.parametrize('name', sorted(zc.hand_cases()))
def test_hand_cases_give_the_numbers_derived_by_hand(name):
    case = zc.hand_cases()[name]
    got, streams, heat = _run_ref(case)
    exp = case['expect']
    S = len(streams)
    if 'line_counts' in exp:
        assert [[tuple(r) for r in got['line_counts'][s, -1].tolist()] for s in range(S)] == exp['line_counts']
    if 'neg_by_frame' in exp:
        assert got['line_counts'][:, :, 0, 1].tolist() == exp['neg_by_frame']
    if 'zone_counts' in exp:
        assert [[tuple(r) for r in got['zone_counts'][s, -1].tolist()] for s in range(S)] == exp['zone_counts']
    for key in ('dwell_sum', 'dwell_max'):
        if key in exp:
            assert [getattr(st, key)[:len(exp[key][s])] for s, st in enumerate(streams)] == exp[key]
    if 'heat' in exp:
        assert np.array_equal(heat, exp['heat'])
    assert [st.now for st in streams] == [case['out']['id'].shape[1]] * S


def test_details_of_the_hand_cases():
    cases = zc.hand_cases()
    got, streams, _ = _run_ref(cases['bad_frame'])
    assert got['inside'][0, 3].tolist() == [0, 0] and got['dwell'][0, 3].reshape(-1).tolist() == [-1, -1] and got['crossed'][0, 3].tolist() == [0, 0]
    assert got['occupancy'][0, :, 0].tolist() == [1, 1, 2, 2, 1, 0, 0]           # the bad frame reports the state's occupancy
    assert got['dwell'][0, 4, 1, 0] == 2 and got['zone_counts'][0, 3].tolist() == got['zone_counts'][0, 2].tolist()
    got, _, _ = _run_ref(cases['reuse'])
    assert got['inside'][0, :, 0].tolist() == [1, 1, 1, 1, 0, 0, 0] and got['dwell'][0, :, 0, 0].tolist() == [0, 1, 0, 1, -1, -1, -1]
    got, _, _ = _run_ref(cases['nonfinite'])
    assert got['inside'][0, :, 0].tolist() == [1, 1, 1, 1, 0, 0, 0] and got['dwell'][0, :4, 0, 0].tolist() == [0, 1, 2, 3]
    got, _, _ = _run_ref(cases['lines'])
    assert got['crossed'][0, 1].tolist() == [2, 2, 0, 0, 0, 0, 0, 0] and got['crossed'][0, 3, 2] == 2 and got['crossed'][1, 1, 0] == 1
    got, _, _ = _run_ref(cases['missed'])
    assert got['crossed'][0, :, 1].tolist() == [0, 0, 0, 0, 2, 0, 0]
    got, _, _ = _run_ref(cases['missed_coasting'])
    assert got['crossed'][0, :, 1].tolist() == [0, 0, 2, 0, 0, 0, 0]
    case = dict(cases['bottom'], zs=dict(cases['bottom']['zs'], anchor='center'))
    assert _run_ref(case)[0]['zone_counts'][0, -1].tolist() == [[0, 0, 0, 0]]


def test_two_calls_equal_one_call():
    for name, splits in (('fuzz', [13, 27]), ('fuzz', [1] * 40), ('fuzz_coasting_bottom', [39, 1]), ('full', [4, 3])):
        case = zc.fuzz_cases()[name]
        one, s_one, h_one = _run_ref(case)
        two, s_two, h_two = _run_ref(case, splits)
        for k in one:
            assert np.array_equal(one[k], two[k]), (name, k)
        for a, b in zip(s_one, s_two):
            for k, v in a.arrays().items():
                assert np.array_equal(v, b.arrays()[k]), (name, k)
        assert (h_one is None and h_two is None) or np.array_equal(h_one, h_two)
    # the fuzz is worth its name: every kind of event happens, and anchors land exactly on edges and lines
    case = zc.fuzz_cases()['fuzz']
    out, streams, heat = _run_ref(case)
    zs = ref.ZoneSet(case['img_hw'], **case['zs'])
    assert all(min(st.entries[:4]) > 0 and min(st.exits[:4]) > 0 and sum(st.lost) > 0 and sum(st.pos) > 0 and sum(st.neg) > 0 for st in streams)
    assert heat.sum() > 100 and (case['out']['count'] < 0).any() and np.isnan(case['out']['box']).any()
    live = case['out']['id'] != 0
    reused = (case['out']['id'][:, 1:] != case['out']['id'][:, :-1]) & live[:, 1:] & live[:, :-1]
    assert reused.sum() > 3
    on_line = 0
    for s, f, t in zip(*np.nonzero(live & (case['out']['missed'] == 0))):
        p = zs.anchor_of(case['out']['box'][s, f, t])
        on_line += p is not None and any(ref.side(line, p) == 0 for line in zs.lines)
    assert on_line > 20


def test_image_objects_carry_the_zone_fields():
    from mydetection_amd.utils.structures import ImageObjects
    n = 5
    o = ImageObjects(torch.arange(n * 4, dtype=torch.float32).view(n, 4), torch.tensor([0, 1, 0, 2, 1]), None, torch.tensor([.1, .5, .3, .9, .2]),
                     'cxcywh', (48, 64), obj_ids=torch.arange(1, n + 1), zone_mask=torch.tensor([1, 0, 3, 2, 0], dtype=torch.int32),
                     line_events=torch.tensor([0, 2, 0, 1, 0], dtype=torch.int32))
    one = o[3]
    assert one.zone_mask.tolist() == [2] and one.line_events.tolist() == [1] and one.obj_ids.tolist() == [4]
    part = o[1:4]
    assert part.zone_mask.tolist() == [0, 3, 2] and part.line_events.tolist() == [2, 0, 1] and part.zone_mask.dtype == torch.int32
    picked = o[torch.tensor([True, False, True, False, True])]
    assert picked.zone_mask.tolist() == [1, 3, 0] and picked.line_events.tolist() == [0, 0, 0]
    o.cpu_()
    assert o.zone_mask.tolist() == [1, 0, 3, 2, 0] and o.line_events.device.type == 'cpu'
    o.sort_by_score_()
    assert o.obj_ids.tolist() == [4, 2, 3, 5, 1] and o.zone_mask.tolist() == [2, 0, 3, 0, 1] and o.line_events.tolist() == [1, 2, 0, 0, 0]
    o.category_filter_([0, 2])
    assert o.obj_ids.tolist() == [4, 3, 1] and o.zone_mask.tolist() == [2, 3, 1] and o.line_events.tolist() == [1, 0, 0]
    plain = ImageObjects(torch.zeros(2, 4), torch.zeros(2, dtype=torch.int64), None, torch.zeros(2))
    assert plain.zone_mask is None and plain.line_events is None and plain[0].zone_mask is None and plain[0].obj_ids is None
    with pytest.raises(AssertionError):
        ImageObjects(torch.zeros(2, 4), torch.zeros(2, dtype=torch.int64), None, torch.zeros(2), zone_mask=torch.zeros(3, dtype=torch.int32))
