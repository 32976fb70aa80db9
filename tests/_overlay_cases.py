"""Synthetic scenes for the counting overlay's tests (no model): what tests/_overlay_ref.frame_ops takes, built by hand or from a
seed, and the trail cases -- tracker outputs of tests/_zones_cases.py with the settings of ops.trail_set.  A scene holds B = 3
frames; the same scene serves S = 1 (F = 3) and S = 3 (F = 1)."""
import functools

import numpy as np

import _zones_cases as zc
import _zones_ref as zr

B = 3
RGB_HW, YUV_HW = (37, 70), (35, 131)          # full and partial 64 x 16 tiles both ways; odd sizes, one full 128-wide tile and a partial one

# a zone partly outside the frame; one with a vertex exactly on a pixel centre (10.5, 8.5); two that share the edge x = 50;
# one that overlaps the others
POLYGONS = [[(-20.0, -10.0), (30.0, -5.0), (25.0, 20.0), (-10.0, 25.0)],
            [(10.5, 8.5), (28.0, 12.0), (20.0, 30.0)],
            [(30.0, 5.0), (50.0, 5.0), (50.0, 30.0), (30.0, 30.0)],
            [(50.0, 5.0), (68.0, 5.0), (68.0, 30.0), (50.0, 30.0)],
            [(20.0, 10.0), (60.0, 12.0), (40.0, 35.0)]]
# one that crosses the tile borders x = 64, y = 16 and y = 32 of the RGB frames; one close to the right edge
LINES = [((2.0, 33.0), (68.0, 3.0)), ((60.25, 0.0), (60.25, 36.0))]
NAMES = ['hall', 'a-name-longer-than-sixteen', 'left', 'right', '', 'door', 'gate']
# frame 0: nobody anywhere; frame 1: some zones occupied; frame 2: multi-digit counters, one beyond 999999
OCCUPANCY = [[0, 0, 0, 0, 0], [1, 0, 2, 0, 7], [12, 345, 0, 9, 10]]
ZONE_COUNTS = [[[0, 0, 0, 0]] * 5,
               [[1, 0, 0, 0], [0, 0, 0, 0], [9, 3, 4, 7], [10, 5, 5, 10], [99, 1, 0, 1]],
               [[1000000, 2, 3, 5], [999999, 0, 0, 0], [100, 50, 49, 99], [12345, 6, 7, 13], [5, 999999, 1, 1000000]]]
LINE_COUNTS = [[[0, 0], [0, 0]], [[3, 9], [10, 0]], [[1000000, 999999], [123456, 654321]]]


def _scene(H, W, polygons=POLYGONS, lines=LINES, names=NAMES, thickness=2, zones=True, lines_on=True,
           counters=('occupancy', 'entries', 'visits'), zone_alpha=48, occupied_alpha=96, trails=None, shift=(0.0, 0.0)):
    sx, sy = W / 70.0 if W > 70 else 1.0, 1.0                            # the wider 4:2:0 frame: the scene stretched over both tiles
    polys = [[(x * sx + shift[0], y * sy + shift[1]) for x, y in poly] for poly in polygons]
    lns = [tuple((x * sx + shift[0], y * sy + shift[1]) for x, y in line) for line in lines]
    return {'img_hw': (H, W), 'pixels': {'polygons': polys, 'lines': lns}, 'polygons': [zr.quantise(p) for p in polys],
            'lines': [tuple(zr.quantise(l)) for l in lns], 'names': list(names), 'thickness': thickness, 'zones': zones, 'lines_on': lines_on,
            'counters': tuple(counters), 'zone_alpha': zone_alpha, 'occupied_alpha': occupied_alpha, 'n_palette': 256, 'label_height': 8,
            'occupancy': OCCUPANCY, 'zone_counts': ZONE_COUNTS, 'line_counts': LINE_COUNTS, 'trails': trails}


def trails(H, W, MT, L, seed, thickness=2, coasting=False, off_frame=False):
    """Random trails of B frames x MT slots: lengths 0 .. L (0 and 1 are not painted), points in and around the frame at 1/16 pixel
    (far outside with off_frame), ids with a large and a negative one, missed -1 (free), 0 and > 0 (coasting)."""
    rng = np.random.default_rng(seed)
    pts = np.zeros((B, MT, L, 2), np.int32)
    lens = rng.integers(0, L + 1, size=(B, MT)).astype(np.int32)
    lens[:, 0] = L                                                       # a full ring in every frame
    missed = rng.choice(np.array([-1, 0, 0, 0, 2], np.int32), size=(B, MT))
    missed[:, 0] = 0
    ids = rng.integers(1, 1000, size=(B, MT)).astype(np.int64)
    ids[:, MT - 1] = (1 << 40) + 77
    if MT > 1:
        ids[:, 1] = -5
    for b in range(B):
        for t in range(MT):
            p = rng.uniform((-8.0, -8.0), (W + 8.0, H + 8.0))
            for k in range(int(lens[b, t])):
                if off_frame:
                    pts[b, t, k] = (zr.q(p[0] + 4 * W), zr.q(p[1] - 3 * H))
                else:
                    pts[b, t, k] = (zr.q(p[0]), zr.q(p[1]))
                p = p + rng.uniform(-9.0, 9.0, size=2)
    free = missed < 0
    lens[free] = 0
    ids[free] = 0
    bbox = np.zeros((B, MT, 4), np.int32)
    for b in range(B):
        for t in range(MT):
            n = int(lens[b, t])
            pts[b, t, n:] = 0
            if n:
                bbox[b, t] = (pts[b, t, :n, 0].min(), pts[b, t, :n, 1].min(), pts[b, t, :n, 0].max(), pts[b, t, :n, 1].max())
    return {'points': pts, 'len': lens, 'bbox': bbox, 'id': ids, 'missed': missed, 'thickness': thickness, 'coasting': coasting}


@functools.lru_cache(maxsize=None)
def scenes(H, W):
    """name -> scene for frames of H x W."""
    no_zone = dict(zones=False, lines_on=False, counters=())
    out = {
        'zones_t1': _scene(H, W, thickness=1),
        'zones_t2': _scene(H, W, thickness=2, counters=('occupancy', 'entries')),
        'zones_t64': _scene(H, W, thickness=64, counters=('visits',)),
        'zones_only': _scene(H, W, lines_on=False, counters=(), zone_alpha=0, occupied_alpha=255),
        'lines_only': _scene(H, W, zones=False, thickness=3),
        'trails2_mt3': _scene(H, W, trails=trails(H, W, 3, 2, 11, thickness=1), **no_zone),
        'trails32_mt64': _scene(H, W, trails=trails(H, W, 64, 32, 12, thickness=2, coasting=True), **no_zone),
        'trails32_mt65': _scene(H, W, trails=trails(H, W, 65, 32, 13, thickness=3), **no_zone),
        'both': _scene(H, W, trails=trails(H, W, 65, 5, 14, coasting=True)),
        'both_no_coasting': _scene(H, W, trails=trails(H, W, 65, 5, 14, coasting=False)),
        # nothing reaches the frame: polygons, lines and labels far below and right of it, trails far right and above
        'nothing': _scene(H, W, thickness=1, counters=(), trails=trails(H, W, 64, 4, 15, off_frame=True), shift=(40.0 * W, 40.0 * H)),
    }
    return out


# ------------------------------------------------------------------------------------------------------------- trail cases
@functools.lru_cache(maxsize=None)
def trail_cases():
    """name -> {'out': tracker outputs, 'ts': the keyword arguments of ops.trail_set}: ring wrap (F = 7 or 40 > L), slot reuse with
    a new id, a bad-class frame, a non-finite anchor, the class filter, anchor='bottom', rotated boxes, 1 .. 512 slots, S = 1 and 3."""
    hand, fuzz = zc.hand_cases(), zc.fuzz_cases()
    walk = zc.blank(1, 40, 2)                                            # 40 frames > L = 32: the full ring wraps; slot 1 changes hands
    zc.path(walk, 0, 0, 11, [(1.0 + 1.5 * f, 40.0 - 0.75 * f) for f in range(40)])
    zc.path(walk, 0, 1, 12, [(60.0 - f, 3.0 + f) for f in range(17)], hold=False)
    zc.path(walk, 0, 1, 13, [(5.0, 5.0 + 0.25 * f) for f in range(23)], f0=17)
    return {
        'walk_L32': {'out': zc.finish(walk), 'ts': dict(max_points=32)},
        'reuse_L2': {'out': hand['reuse']['out'], 'ts': dict(max_points=2)},
        'reuse_L32': {'out': hand['reuse']['out'], 'ts': dict(max_points=32)},
        'bad_frame': {'out': hand['bad_frame']['out'], 'ts': dict(max_points=3)},
        'nonfinite': {'out': hand['nonfinite']['out'], 'ts': dict(max_points=4)},
        'classes': {'out': hand['classes']['out'], 'ts': dict(max_points=3, classes=[1, 7])},
        'bottom': {'out': hand['bottom']['out'], 'ts': dict(max_points=5, anchor='bottom')},
        'rotated': {'out': hand['rotated']['out'], 'ts': dict(max_points=2)},
        'lines': {'out': hand['lines']['out'], 'ts': dict(max_points=4)},
        'fuzz_L7': {'out': fuzz['fuzz']['out'], 'ts': dict(max_points=7)},
        'fuzz_L32': {'out': fuzz['fuzz']['out'], 'ts': dict(max_points=32)},
        'fuzz_L32_classes': {'out': fuzz['fuzz']['out'], 'ts': dict(max_points=32, classes=[0, 2])},
        'mt1': {'out': fuzz['mt1']['out'], 'ts': dict(max_points=2)},
        'mt512': {'out': fuzz['mt512']['out'], 'ts': dict(max_points=6)},
    }
