"""Synthetic tracker outputs for the zone and line counting tests (no model): the arrays ops.track_frames returns, built by hand
or from a seed.  A case is a dict: img_hw, zs (the keyword arguments of ops.zone_set / _zones_ref.ZoneSet besides img_hw), out
(box [S,F,MT,5] float32, id, cls int64, missed int32 [S,F,MT], count int32 [S,F]) and expect (hand-derived final numbers per
stream, checked on the restatement by tests/test_zones_host.py; the GPU test holds the kernel to the restatement)."""
import math

import numpy as np

BAD_CLASS = -1
F_HAND = 7
LINE = ((10.0, 10.0), (10.0, 30.0))          # x = 10, directed towards +y: x < 10 is its positive side
SQUARE = ((0.0, 0.0), (20.0, 0.0), (20.0, 20.0), (0.0, 20.0))


def blank(S, F, MT):
    return {'box': np.zeros((S, F, MT, 5), np.float32), 'id': np.zeros((S, F, MT), np.int64), 'cls': np.zeros((S, F, MT), np.int64),
            'missed': np.full((S, F, MT), -1, np.int32), 'count': np.zeros((S, F), np.int32)}


def put(out, s, f, slot, tid, xy, wh=(4.0, 6.0), ang=0.0, cls=0, missed=0):
    out['box'][s, f, slot] = (xy[0], xy[1], wh[0], wh[1], ang)
    out['id'][s, f, slot], out['cls'][s, f, slot], out['missed'][s, f, slot] = tid, cls, missed


def path(out, s, slot, tid, pts, f0=0, hold=True, **kw):
    """One track over consecutive frames from f0; with hold it stays at its last point to the end of the call."""
    F = out['id'].shape[1]
    for f in range(f0, F):
        k = f - f0
        if k >= len(pts) and not hold:
            break
        put(out, s, f, slot, tid, pts[min(k, len(pts) - 1)], **kw)


def bad_frame(out, s, f):
    """What the tracker writes for a bad-class frame: free slots and the sentinel."""
    out['box'][s, f] = 0
    out['id'][s, f] = 0
    out['cls'][s, f] = 0
    out['missed'][s, f] = -1
    out['count'][s, f] = BAD_CLASS


def finish(out):
    live = (out['id'] != 0).sum(axis=2).astype(np.int32)
    out['count'] = np.where(out['count'] == BAD_CLASS, out['count'], live).astype(np.int32)
    return out


def case_lines():
    """Every way of meeting one line: through A and through B exactly, touched for two frames and continued, touched and
    returned, around its end, walked along.  Stream 0 goes from the positive to the negative side, stream 1 the other way,
    stream 2 holds one track that goes to and fro."""
    ways = [[(5, 10), (15, 10)], [(5, 30), (15, 30)], [(5, 20), (10, 20), (10, 22), (15, 22)], [(5, 24), (10, 24), (10, 26), (5, 26)],
            [(5, 35), (15, 35)], [(10, 12), (10, 15), (10, 25), (12, 25)]]
    out = blank(3, F_HAND, 8)
    for slot, pts in enumerate(ways):
        path(out, 0, slot, slot + 1, pts)
        path(out, 1, slot, slot + 1, [(20 - x, y) for x, y in pts])
    path(out, 2, 3, 9, [(5, 20), (15, 20)] * 3 + [(5, 20)])
    return {'img_hw': (48, 64), 'zs': {'lines': [LINE]}, 'out': finish(out),
            'expect': {'line_counts': [[(0, 3)], [(3, 0)], [(3, 3)]]}}


def case_missed(coasting):
    """A track crosses while it is missed for three frames: counted at the re-match, or with coasting where the prediction crosses."""
    out = blank(1, F_HAND, 2)
    for f, (x, m) in enumerate([(5, 0), (8, 1), (11, 2), (14, 3), (17, 0), (18, 0), (19, 0)]):
        put(out, 0, f, 1, 7, (x, 20), missed=m)
    first = 2 if coasting else 4
    return {'img_hw': (48, 64), 'zs': {'lines': [LINE], 'coasting': coasting}, 'out': finish(out),
            'expect': {'line_counts': [[(0, 1)]], 'neg_by_frame': [[int(f >= first) for f in range(F_HAND)]]}}


def _reuse_out():
    out = blank(1, F_HAND, 2)
    path(out, 0, 0, 1, [(10, 10), (11, 11)], hold=False)                          # dies inside; its slot is taken at once
    path(out, 0, 0, 2, [(12, 12), (12, 13)], f0=2, hold=False)                    # dies inside; the slot stays free
    path(out, 0, 1, 3, [(30, 30), (30, 30), (10, 5), (10, 6), (10, 7), (30, 30)])
    return out


def case_reuse():
    """Slot reuse: a track dies inside and a new id is born in the same slot in the next frame; another walks in and out."""
    return {'img_hw': (48, 64), 'zs': {'polygons': [SQUARE]}, 'out': finish(_reuse_out()),
            'expect': {'zone_counts': [[(3, 1, 2, 3)]], 'dwell_sum': [[7]], 'dwell_max': [[3]]}}


def case_bad_frame():
    """The same with a bad-class frame in the middle: the state stands, the frame counter goes on."""
    out = _reuse_out()
    bad_frame(out, 0, 3)
    return {'img_hw': (48, 64), 'zs': {'polygons': [SQUARE]}, 'out': finish(out),
            'expect': {'zone_counts': [[(3, 1, 2, 3)]], 'dwell_sum': [[7]], 'dwell_max': [[3]]}}


def case_classes():
    out = blank(1, F_HAND, 3)
    path(out, 0, 0, 1, [(30, 30), (10, 10)], cls=0)
    path(out, 0, 1, 2, [(30, 30), (30, 30), (10, 12)], cls=1)
    path(out, 0, 2, 3, [(10, 14)], cls=5)
    return {'img_hw': (48, 64), 'zs': {'polygons': [SQUARE], 'classes': [1, 7]}, 'out': finish(out),
            'expect': {'zone_counts': [[(1, 0, 0, 0)]]}}


def case_bottom():
    """anchor='bottom': the centre stays above the polygon, the foot point walks in."""
    out = blank(1, F_HAND, 1)
    path(out, 0, 0, 1, [(10, 15), (10, 15.5), (10, 16), (10, 12)], wh=(4.0, 9.0))  # foot at 19.5, 20.0 (on the edge), 20.5, 16.5
    poly = [(0, 20), (20, 20), (20, 40), (0, 40)]
    return {'img_hw': (48, 64), 'zs': {'polygons': [poly], 'anchor': 'bottom'}, 'out': finish(out),
            'expect': {'zone_counts': [[(1, 1, 0, 1)]], 'dwell_sum': [[2]]}}


def case_rotated():
    """5-wide rotated boxes: the angle column is carried and not read."""
    out = blank(1, F_HAND, 2)
    path(out, 0, 0, 1, [(30, 30), (10, 10)], ang=33.5)
    path(out, 0, 1, 2, [(10, 12)], ang=179.0)
    return {'img_hw': (48, 64), 'zs': {'polygons': [SQUARE]}, 'out': finish(out), 'expect': {'zone_counts': [[(2, 0, 0, 0)]]}}


def case_nonfinite():
    """A NaN or an infinity in the anchor: unobserved in that frame, the state stands and the dwell goes on."""
    out = blank(1, F_HAND, 1)
    path(out, 0, 0, 4, [(10, 10), (float('nan'), 10), (10, float('inf')), (10, float('-inf')), (30, 30)])
    return {'img_hw': (48, 64), 'zs': {'polygons': [SQUARE]}, 'out': finish(out),
            'expect': {'zone_counts': [[(1, 1, 0, 1)]], 'dwell_sum': [[4]]}}


def case_heat():
    """Heat cells of an 8 x 12 pixel grid on a 64 x 48 frame: at a cell boundary, just below it, at x = W exactly, at negative
    coordinates, and a coasting track (observed, but never heated)."""
    pts = [(8.0, 12.0), (7.99, 11.99), (64.0, 10.0), (63.99, 47.99), (-0.01, 5.0), (5.0, -3.0), (0.0, 0.0), (16.0, 47.99), (10.0, 48.0)]
    out = blank(1, 1, 16)
    for slot, p in enumerate(pts):
        put(out, 0, 0, slot, slot + 1, p)
    put(out, 0, 0, 12, 20, (40.0, 40.0), missed=2)
    want = np.zeros((1, 4, 8), np.int32)
    for cy, cx in [(1, 1), (0, 0), (3, 7), (0, 0), (3, 2)]:
        want[0, cy, cx] += 1
    return {'img_hw': (48, 64), 'zs': {'lines': [LINE], 'heat': (4, 8), 'coasting': True}, 'out': finish(out), 'expect': {'heat': want}}


def star(cx, cy, r_out, r_in, n=16, phase=0.0):
    """A concave n-gon around (cx, cy), vertices snapped to 1/4 pixel."""
    return [(round((cx + (r_out if i % 2 == 0 else r_in) * math.cos(phase + 2 * math.pi * i / n)) * 4) / 4,
             round((cy + (r_out if i % 2 == 0 else r_in) * math.sin(phase + 2 * math.pi * i / n)) * 4) / 4) for i in range(n)]


FUZZ_POLYGONS = [[(8, 8), (32, 8), (32, 40), (8, 40)], [(32, 8), (56, 8), (56, 40), (32, 40)],     # two squares that share an edge
                 [(0, 0), (48, 0), (0, 48)], [(10, 10), (50, 10), (50, 40), (30, 20), (10, 40)]]   # a diagonal edge; a concave one
FUZZ_LINES = [((32, 0), (32, 48)), ((0, 0), (48, 48)), ((20, 24), (44, 24)), ((64, 0), (16, 48))]


def full_zone_set(seed=5):
    """16 polygons of 16 vertices and 16 lines on a 64 x 48 frame."""
    rng = np.random.RandomState(seed)
    polys = [star(rng.uniform(8, 56), rng.uniform(8, 40), rng.uniform(8, 20), rng.uniform(2, 7), 16, rng.uniform(0, 1)) for _ in range(16)]
    lines = []
    while len(lines) < 16:
        a, b = rng.randint(0, 64, 2), rng.randint(0, 64, 2)
        if (a != b).any():
            lines.append(((float(a[0]), float(a[1] * 0.75)), (float(b[0]), float(b[1] * 0.75))))
    return polys, lines


def fuzz_out(seed, S, F, MT, img_hw=(48, 64), p_born=0.15, p_die=0.06, p_bad=0.05):
    """Random walks with births, deaths, slots reused in the frame of a death, missed frames, a few NaNs and bad-class frames.
    Coordinates are multiples of 1/32 pixel and often whole pixels, so many anchors land exactly on edges and lines."""
    rng = np.random.RandomState(seed)
    H, W = img_hw
    out = blank(S, F, MT)
    for s in range(S):
        next_id = 1
        tid = np.zeros(MT, np.int64)
        pos = np.zeros((MT, 2))
        cls = np.zeros(MT, np.int64)
        missed = np.zeros(MT, np.int32)
        born_scale = p_born * (0.3 + 0.7 * s / max(S - 1, 1))      # the streams differ in how crowded they are
        for f in range(F):
            for t in range(MT):
                reuse = False
                if tid[t] != 0 and rng.rand() < p_die:
                    tid[t] = 0
                    reuse = rng.rand() < 0.3                         # a new id in the same slot in the frame of the death
                    if not reuse:
                        continue
                if tid[t] == 0:
                    if reuse or rng.rand() < born_scale:
                        tid[t], next_id = next_id, next_id + 1
                        pos[t] = rng.uniform(-4, W + 4), rng.uniform(-4, H + 4)
                        cls[t], missed[t] = rng.randint(0, 3), 0
                    else:
                        continue
                else:
                    pos[t] += rng.uniform(-6, 6, 2)
                    missed[t] = missed[t] + 1 if rng.rand() < 0.2 else 0
                pos[t] = np.round(pos[t]) if rng.rand() < 0.4 else np.round(pos[t] * 32) / 32
                x, y = pos[t]
                if rng.rand() < 0.01:
                    x = float('nan')
                put(out, s, f, t, tid[t], (x, y), wh=(rng.randint(2, 9), rng.randint(2, 9)), ang=rng.uniform(0, 180), cls=cls[t],
                    missed=missed[t])
            if 0 < f and rng.rand() < p_bad:
                bad_frame(out, s, f)
    return finish(out)


def hand_cases():
    return {'lines': case_lines(), 'missed': case_missed(False), 'missed_coasting': case_missed(True), 'reuse': case_reuse(),
            'bad_frame': case_bad_frame(), 'classes': case_classes(), 'bottom': case_bottom(), 'rotated': case_rotated(),
            'nonfinite': case_nonfinite(), 'heat': case_heat()}


def fuzz_cases():
    polys, lines = full_zone_set()
    hw = (48, 64)
    walk = fuzz_out(11, 3, F_HAND, 65, hw, p_born=0.5)
    return {
        'fuzz': {'img_hw': hw, 'zs': {'polygons': FUZZ_POLYGONS, 'lines': FUZZ_LINES, 'heat': (6, 8)}, 'out': fuzz_out(1, 3, 40, 65, hw)},
        'fuzz_coasting_bottom': {'img_hw': hw, 'zs': {'polygons': FUZZ_POLYGONS, 'lines': FUZZ_LINES, 'coasting': True, 'anchor': 'bottom',
                                                      'classes': [0, 2]}, 'out': fuzz_out(2, 3, 40, 65, hw)},
        'full': {'img_hw': hw, 'zs': {'polygons': polys, 'lines': lines, 'heat': (5, 7)}, 'out': walk},
        'polygons_only': {'img_hw': hw, 'zs': {'polygons': polys}, 'out': walk},
        'lines_only': {'img_hw': hw, 'zs': {'lines': lines}, 'out': walk},
        'mt1': {'img_hw': hw, 'zs': {'polygons': FUZZ_POLYGONS, 'lines': FUZZ_LINES, 'heat': (3, 4)}, 'out': fuzz_out(3, 3, F_HAND, 1, hw, p_born=0.9, p_die=0.2)},
        'mt512': {'img_hw': hw, 'zs': {'polygons': FUZZ_POLYGONS, 'lines': FUZZ_LINES, 'heat': (12, 16)}, 'out': fuzz_out(4, 3, F_HAND, 512, hw, p_born=0.3)},
    }
