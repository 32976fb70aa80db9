"""Crafted inputs of the fusion of view records (tests/test_tta_host.py, tests/test_gpu_tta.py).  No GPU, no package import.

A case is a dict: boxes [V,512,W] float32 in the pixel coordinates of each MIRRORED frame, scores [V,512], cats [V,512],
counts [V], flips [V], frame_hw, thres, and optionally agnostic / min_score.  Slots past a view's count hold poison (a score of
2 and a box that covers everything) that no fusion may read."""
import numpy as np

F32 = np.float32
FRAME = (300, 400)


def _blank(V, width=4):
    b = np.zeros((V, 512, width), F32)
    b[:, :, 2:4] = 10000
    return b, np.full((V, 512), 2.0, F32), np.full((V, 512), 1, np.int64)


def case(rows, flips, thres, frame_hw=FRAME, width=4, counts=None, **kw):
    """rows: per view a list of (box in FRAME coordinates, score, class); the box is stored mirrored into its view (exact for
    the integer and quarter coordinates the crafted cases use)."""
    V = len(flips)
    b, s, c = _blank(V, width)
    H, W = frame_hw
    for v, (view, f) in enumerate(zip(rows, flips)):
        for k, (box, score, cat) in enumerate(view):
            box = list(box)
            if f & 1:
                box[0] = W - box[0]
            if f & 2:
                box[1] = H - box[1]
            if width == 5 and f in (1, 2):
                box[4] = -box[4]
            b[v, k], s[v, k], c[v, k] = box, score, cat
    counts = [len(view) for view in rows] if counts is None else list(counts)
    return dict(boxes=b, scores=s, cats=c, counts=counts, flips=list(flips), frame_hw=frame_hw, thres=thres, **kw)


def random_clusters(seed, V, width=4, n_obj=30, n_cls=3, seen=0.8, frame_hw=FRAME, thres=0.55, counts=None, jitter=2.0, flips=None, **kw):
    """Objects at shared frame positions, each seen by a view with probability `seen` as a jittered box with a score of its own
    (all scores distinct); every view has a flip (random when `flips` is None) and keeps its boxes in its own mirrored
    coordinates.  counts: the number of boxes of every view instead of `seen`."""
    rng = np.random.Generator(np.random.PCG64(seed))
    H, W = frame_hw
    ctr = np.stack([rng.uniform(20, W - 20, n_obj), rng.uniform(20, H - 20, n_obj)], 1)
    wh = rng.uniform(14, 70, size=(n_obj, 2))
    ang = rng.uniform(-90, 90, size=n_obj)
    kc = rng.integers(0, n_cls, size=n_obj)
    drawn = [int(f) for f in rng.integers(0, 4, size=V)]
    if V > 1:
        drawn[0], drawn[1] = 0, 1
    flips = drawn if flips is None else list(flips)
    b, s, c = _blank(V, width)
    pool = rng.permutation(np.linspace(0.05, 0.95, V * 512)).astype(F32).reshape(V, 512)
    made = []
    for v in range(V):
        objs = [k for k in range(n_obj) if rng.random() < seen] if counts is None else list(rng.integers(0, n_obj, size=counts[v]))
        made.append(len(objs))
        for slot, k in enumerate(objs):
            box = np.concatenate([ctr[k] + rng.normal(0, jitter, 2), wh[k] * (1 + rng.normal(0, 0.05, 2)), [ang[k] + rng.normal(0, 5)]])
            if flips[v] & 1:
                box[0] = W - box[0]
            if flips[v] & 2:
                box[1] = H - box[1]
            if flips[v] in (1, 2):
                box[4] = -box[4]
            b[v, slot], s[v, slot], c[v, slot] = box[:width], pool[v, slot], kc[k]
    return dict(boxes=b, scores=s, cats=c, counts=made, flips=flips, frame_hw=frame_hw, thres=thres, **kw)


def grid_over_the_cap(seed=4):
    """More than 512 clusters: two views of 512 boxes each on a grid of 1 000 separate cells, so about 1 000 boxes found their own
    cluster or try to; the last 40 boxes of view 1 sit on cells of view 0's best boxes with the lowest scores of all, so they JOIN
    clusters after the cap is met, while the singletons around them in order P are dropped."""
    rng = np.random.Generator(np.random.PCG64(seed))
    V = 2
    b, s, c = _blank(V)
    cells = rng.permutation(1000)
    scores = rng.permutation(np.linspace(0.2, 0.95, 1024)).astype(F32)
    for v in range(V):
        for k in range(512):
            cell = cells[(v * 512 + k) % 1000]
            b[v, k] = (5 + 10 * (cell % 40), 5 + 10 * (cell // 40), 8, 8)
            s[v, k], c[v, k] = scores[v * 512 + k], cell % 2
    top = np.argsort(-s[0])[:40]
    for i, k in enumerate(top):
        b[1, 472 + i] = b[0, k] + np.array([0.5, 0, 0, 0], F32)
        s[1, 472 + i], c[1, 472 + i] = F32(0.01 + 0.001 * i), c[0, k]
    return dict(boxes=b, scores=s, cats=c, counts=[512, 512], flips=[0, 0], frame_hw=(300, 400), thres=0.5)


def crafted_wbf():
    """name -> case: the edge rules of MYDET_FUSE_WBF."""
    A, B_, C = (100, 100, 20, 20), (104, 100, 20, 20), (300, 200, 40, 30)
    out = {}
    # one object seen by two views with EQUAL scores, and one seen once
    out['equal scores'] = case([[(A, 0.5, 0), (C, 0.5, 1)], [(A, 0.5, 0)]], [0, 1], 0.5)
    # a candidate equidistant from two clusters: IoU 0.2 with both; the cluster founded first (the higher score, at x = 130) gets it
    out['equidistant'] = case([[((130, 50, 10, 10), 0.9, 0), ((110, 50, 10, 10), 0.8, 0)], [((120, 50, 20, 10), 0.7, 0)]], [0, 3], 0.1)
    out['equidistant, founders exchanged'] = case([[((130, 50, 10, 10), 0.8, 0), ((110, 50, 10, 10), 0.9, 0)], [((120, 50, 20, 10), 0.7, 0)]],
                                                  [0, 2], 0.1)
    # a chain: B joins A (IoU 6/14) and moves the fused row to cx = 52; C overlaps that row (5/15) above 0.3, the founder (3/17) below
    out['chain'] = case([[((50, 50, 10, 10), 0.9, 0)], [((54, 50, 10, 10), 0.9, 0)], [((57, 50, 10, 10), 0.5, 0)]], [0, 1, 2], 0.3)
    # boxes without area on one spot: 0/0, NaN, never a match -- three clusters; and a box of width 0 beside a real one
    out['zero areas'] = case([[((70, 50, 0, 20), 0.9, 0), (A, 0.6, 0)], [((70, 50, 0, 20), 0.8, 0), ((70, 50, 0, 0), 0.7, 0)]], [0, 1], 0.0)
    # empty views, and scores that are not > 0 inside the count
    out['empty views'] = case([[], [(A, 0.7, 2)], []], [1, 0, 3], 0.5)
    out['no candidates'] = case([[], []], [0, 1], 0.5)
    out['scores not above zero'] = case([[(A, 0.0, 0), (C, -0.5, 0), (B_, 0.4, 0)], [(A, -0.0, 0), (C, 0.3, 1)]], [0, 1], 0.5)
    # min_score: V = 3, a singleton scores s / 3
    rows = [[(A, 0.9, 0), (C, 0.9, 0)], [(B_, 0.8, 0)], [(A, 0.7, 0), ((30, 30, 10, 10), 0.59, 1), ((200, 30, 10, 10), 0.61, 1)]]
    out['min_score cuts singletons'] = case(rows, [0, 1, 2], 0.4, min_score=0.2)
    out['min_score zero keeps them'] = case(rows, [0, 1, 2], 0.4)
    # agnostic: two classes on one spot are one cluster with the first member's class; class-aware they are two
    two = [[(A, 0.9, 3), (C, 0.5, 1)], [(B_, 0.8, 1), (C, 0.6, 2)]]
    out['two classes, class-aware'] = case(two, [0, 1], 0.4)
    out['two classes, agnostic'] = case(two, [0, 1], 0.4, agnostic=True)
    return out


def permuted(c, perm):
    """The case with its views in another order."""
    perm = list(perm)
    return dict(c, boxes=c['boxes'][perm], scores=c['scores'][perm], cats=c['cats'][perm], counts=[c['counts'][v] for v in perm],
                flips=[c['flips'][v] for v in perm])


def fields(c):
    return c['boxes'], c['scores'], c['cats'], c['counts'], c['flips'], c['frame_hw'], c['thres']
