"""The cases of the fused-cost tests (test code): hand-made records and descriptors for mydet_track_frames_appear_optimal_f32.
tests/test_appear_cost_host.py asserts on the restatement alone what the GPU tests rely on: the margins of every case and the
outcome each case is for."""
import functools

import numpy as np

import _appear_cases as base
from _appear_cases import BLUE, GREEN, MIXED, RED, _fr, pack_desc

TRACK_HW = base.TRACK_HW
BANDS = base.BANDS
W, H = 40.0, 60.0


def level(v):
    return base.level(v)


# ---- the swap: two objects of one class cross between two frames ----

def swap(width=4, neighbour=False):
    """Tracks at x = 200 and 216 (IoU 0.43 with each other's box), three frames standing.  In the last frame the first object is
    detected at 212 and the second at 204: IoU 0.54 with its own prediction, 0.82 with the other's, so the pairing of largest
    total IoU is the swapped one.  The first object is RED; the second BLUE, or with neighbour=True MIXED: S = 65536 against a
    RED template and back, which passes the default gate of 0.3.  (frames, descs)."""
    other = MIXED if neighbour else BLUE
    fr, ds = [], []
    for f in range(3):
        fr.append(_fr([((200.0, 200.0, W, H, 0.0), 0.9, 0), ((216.0, 200.0, W, H, 0.0), 0.8, 0)], width))
        ds.append([RED, other])
    # the better score on the second object: the greedy walk lets it choose first
    fr.append(_fr([((204.0, 200.0, W, H, 0.0), 0.95, 0), ((212.0, 200.0, W, H, 0.0), 0.7, 0)], width))
    ds.append([other, RED])
    return fr, pack_desc(ds)


def painted_swap(hw=(240, 320)):
    """The swap as a video: uint8 frames [4, H, W, 3] on grey and the rotated records (angle 0) of two 40 x 60 boxes, the second
    16 px lower than the first, as frames for _track_ref.pack_records.  The first object carries a RED band in the 16 rows
    above the second one's samples, the second a BLUE band in the 16 rows below the first one's: the boxes overlap, but neither
    descriptor ever sees the other's colour.  Three frames standing at x = 100 and 121 (IoU 0.21), then the first is detected
    at 118 and the second at 103: IoU 0.38 with its own prediction, 0.51 with the other's.  The descriptors come from the pixels."""
    frames = np.full((4, hw[0], hw[1], 3), 128, np.uint8)
    ya, yb = 120, 136
    recs = []
    for f, (xa, xb) in enumerate([(100, 121)] * 3 + [(118, 103)]):
        frames[f, ya - 24:ya - 8, xa - 20:xa + 20] = (255, 0, 0)
        frames[f, yb + 8:yb + 24, xb - 20:xb + 20] = (0, 0, 255)
        recs.append(_fr([((float(xa), float(ya), W, H, 0.0), 0.9, 0), ((float(xb), float(yb), W, H, 0.0), 0.8, 0)], 5))
    return frames, recs


# ---- shapes: pairs of neighbours on a grid, F = 4 ----

GRID_NS = {1: (1, 2, 0, 1), 64: (63, 64, 65, 0), 65: (1, 65, 64, 65), 512: (65, 512, 512, 63)}


def obj_desc(i, f):
    """The descriptor of object i in frame f: three bins of its own, a little of it moving with the frame (templates blend)."""
    d = np.zeros(128, np.uint16)
    b = (5 * i) % 128
    d[b], d[(b + 64) % 128], d[(b + 1) % 128] = 300 - 6 * f, 6 * f, 212
    return d


def grid_box(i, f):
    """Object i of the grid in frame f: clusters of two 12 x 16 boxes 4 px apart (IoU 0.5), 40 x 30 px between clusters (IoU 0),
    every object drifting by half a pixel per frame."""
    c = i // 2
    return (20.0 + 40.0 * (c % 16) + (2.0 if i % 2 else -2.0) + 0.5 * f, 15.0 + 30.0 * (c // 16), 12.0, 16.0, 0.0)


def grid(ns, width=4, seed=9):
    """F = len(ns) frames; frame f holds the objects 0 .. ns[f] - 1 in a shuffled record order, scores falling with the index.
    (frames, descs)"""
    rng = np.random.Generator(np.random.PCG64(seed))
    fr, ds = [], []
    for f, n in enumerate(ns):
        order = rng.permutation(n)
        fr.append(_fr([(grid_box(int(i), f), 0.9 - 0.0005 * int(i), 0) for i in order], width))
        ds.append([obj_desc(int(i), f) for i in order])
    return fr, pack_desc(ds)


def crowd(width=4):
    """70 grid objects and, ranked behind them, a crowd of 20 boxes of 40 x 60 within a few pixels of each other (pairwise IoU >
    0.6), born into the slots 70 .. 89 in frame 0.  In each later frame ONE of the crowd is detected: 20 needed pairs in one
    64-slot chunk (the dense form of the similarity phase), one row against 20 columns in the solve.  (frames, descs)"""
    def crowd_box(k):
        return (300.0 + 1.5 * (k % 5 - 2), 400.0 + 1.5 * (k // 5 - 1.5), W, H, 0.0)
    fr, ds = [], []
    for f, seen in enumerate((range(20), (7,), (12,), (3,))):
        rows = [(grid_box(i, f), 0.9 - 0.0005 * i, 0) for i in range(70)] + [(crowd_box(k), 0.8 - 0.001 * k, 0) for k in seen]
        fr.append(_fr(rows, width))
        ds.append([obj_desc(i, f) for i in range(70)] + [obj_desc(200 + k, f) for k in seen])
    return fr, pack_desc(ds)


# ---- instances and settings: the busy scene of the appearance tests and two more objects ----

def settings(width, bands, rot, gate):
    """_appear_cases.busy (six drifting objects of two classes, one lost and back with a jump -- the re-identification --, one in
    the low band from frame 4 on, a bad-class frame at 3, a newcomer at 5) and
      * with a gate: a RED object of class 1 at (560, 100) that turns GREEN in frame 5 -- S = 0, a pair that only the gate removes;
      * with bands: from frame 4 on a second, low-band detection 8 px beside object 0, whose track the first stage has taken --
        ineligible in stage 2 though its S is needed.
    (frames, descs)"""
    fr, ds = base.busy(width, low=bands, rot=rot)
    fr, ds = list(fr), ds.copy()

    def add(f, box, score, cat, desc):
        b, s, c = fr[f]
        ds[f, len(s)] = desc
        fr[f] = (np.concatenate([b, np.array([box[:width]], np.float32)]), np.append(s, np.float32(score)), np.append(c, np.int64(cat)))
    for f in range(len(fr)):
        if fr[f] is None:
            continue
        first = tuple(float(v) for v in fr[f][0][0]) + ((0.0,) if width == 4 else ())
        if gate:
            add(f, (560.0, 100.0, 30.0, 40.0, 0.0), 0.62, 1, GREEN if f >= 5 else RED)
        if bands and f >= 4:
            add(f, (first[0] + 8.0,) + first[1:5], 0.35, 0, ds[f, 0])
    return fr, ds


VARIANTS = {'bw4': dict(width=4, match='iou'), 'bw5': dict(width=5, match='iou'), 'rot': dict(width=5, match='rotated')}
# (variant, bands, shift, gate, reid, weight): every instance, every setting on and off, every weight
SETTINGS = [('bw4', False, False, 0.0, 0.0, 0), ('bw4', True, True, 0.3, 0.5, 128), ('bw5', False, True, 0.3, 0.0, 256),
            ('bw5', True, False, 0.0, 0.5, 128), ('rot', False, False, 0.3, 0.5, 128), ('rot', True, True, 0.3, 0.5, 256),
            ('rot', True, False, 0.0, 0.0, 0)]


def shifts_of(n):
    sh = np.zeros((n, 4), np.int32)
    sh[1], sh[2] = (3, 1, 1, 9), (-2, 2, 0, 9)                       # the second one is not valid: nothing moves
    return sh


def moved(frames, sh, width):
    """The frames with every box moved by the valid shifts so far: the scene a moving camera sees."""
    if sh is None:
        return frames
    cum = np.cumsum(sh[:, :2] * sh[:, 2:3], axis=0)
    return [fr if fr is None else (fr[0] + np.pad(cum[f], (0, width - 2)).astype(np.float32), fr[1], fr[2]) for f, fr in enumerate(frames)]


def appear_kw(gate, reid):
    """(the keywords of ops.appear_set, those of the restatement's Stream) of one setting."""
    a = dict(gate=gate or None, reid=reid or None, momentum=0.8, reach=2.0, update_thres=0.5)
    r = dict(gate=level(gate), reid=level(reid), alpha=51, reach=2.0, update_thres=0.5)      # alpha = floor(0.2 * 256 + 0.5)
    return a, r


@functools.lru_cache(maxsize=None)
def restated(name, *key):
    """The restatement of a case, computed once per process and shared: (frames, descs, stream, outs, arrays).  The callers leave
    all of it unchanged."""
    import _appear_cost_ref as ref
    if name == 'grid':
        mt, = key
        frames, descs = grid(GRID_NS[mt])
        out = ref.run(frames, descs, 4, TRACK_HW, mt, appear=appear_kw(0.3, 0.0)[1], weight=128)
    elif name == 'crowd':
        frames, descs = crowd()
        out = ref.run(frames, descs, 4, TRACK_HW, 128, appear=appear_kw(0.0, 0.0)[1], weight=128)
    elif name == 'swap':
        neighbour, weight = key
        frames, descs = swap(4, neighbour)
        out = ref.run(frames, descs, 4, TRACK_HW, 64, appear=appear_kw(0.3, 0.6)[1], weight=weight)
    else:
        variant, bands, shift, gate, reid, weight = key
        v = VARIANTS[variant]
        frames, descs = settings(v['width'], bands, variant == 'rot', gate > 0)
        sh = shifts_of(len(frames)) if shift else None
        frames = moved(frames, sh, v['width'])
        out = ref.run(frames, descs, v['width'], TRACK_HW, 64, params=dict(match=v['match']), appear=appear_kw(gate, reid)[1],
                      assoc=BANDS if bands else None, shifts=sh, weight=weight)
    return (frames, descs) + out
