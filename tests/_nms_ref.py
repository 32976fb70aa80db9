"""The NMS modes of include/mydet.h ("NMS modes") restated in numpy, for tests/test_nms_modes_host.py and
tests/test_gpu_nms_modes.py.  No GPU, no package import.

Every pair value o is a float32 scalar computed in the kernel's operation order; the picks, the decay and the merge are plain
Python loops in order P.  The Gaussian weight is np.float32(np.exp(-(np.float64(o) * np.float64(o)) / sigma)): the square of a
float32 is exact in float64, the quotient is correctly rounded, and only exp may differ between two correct libraries -- by an
ulp of float64.  `Stats.midpoint` says how far that leaves every weight from a float32 rounding midpoint, which is what makes
`==` against another exp legitimate; `Stats.gap` is the smallest relative distance between the two largest working scores at a
pick (reported, not required: a tie is resolved by the candidate index).

    out = run(b, c, s, conf, thr, kind, agnostic=False, sigma=0.5, min_score=None, topk=512, stats=None)
    out['count'], out['index'] [K], out['cls'] [K], out['score'] [K] float32, out['bbox'] [K, 4 or 5] float32
"""
import numpy as np

F32 = np.float32
KINDS = ('hard', 'soft-linear', 'soft-gaussian', 'merge')


class Stats:
    """What a run met: see the module docstring.  One object may collect several runs."""

    def __init__(self):
        self.midpoint = np.inf        # smallest relative distance of a Gaussian weight (float64) from a float32 rounding midpoint
        self.gap = np.inf             # smallest relative gap between the two largest working scores at a pick (ties excluded)
        self.weights = 0              # Gaussian weights computed with o != 0
        self.reordered = 0            # groups whose emission order is not order P
        self.cross_class = 0          # agnostic: pairs of different classes where one suppressed / decayed / absorbed the other
        self.merged = 0               # merge: kept boxes whose cluster holds more than themselves
        self.cut = 0                  # soft: groups stopped by min_score with boxes left


def select(c, s, conf, topk=512):
    """Candidate indices of the selected list in order P over all classes (score descending, index ascending; -0 and +0 tie),
    and whether one of them has a class id outside [0, 4096)."""
    s = np.asarray(s, F32)
    with np.errstate(invalid='ignore'):
        sel = np.nonzero(s >= F32(conf))[0]                       # a NaN score, or a NaN conf, passes nothing
    sel = sel[np.argsort(-(s[sel] + F32(0)), kind='stable')][:topk]           # -0 + 0 = +0: the two zeros tie
    cls = np.asarray(c, np.int64)[sel]
    return sel, bool(((cls < 0) | (cls > 4095)).any())


def corners(b):
    """x1, y1, x2, y2 and the area of rows (cx, cy, w, h, ...) in float32, as postprocess.hip computes them."""
    b = np.asarray(b, F32)
    hw, hh = b[:, 2] / F32(2), b[:, 3] / F32(2)
    x1, y1, x2, y2 = b[:, 0] - hw, b[:, 1] - hh, b[:, 0] + hw, b[:, 1] + hh
    return x1, y1, x2, y2, (x2 - x1) * (y2 - y1)


def pair_matrix(b):
    """o(i, j) of every pair of rows, float32 [n, n]: inter / (a_i + a_j - inter), 0/0 = NaN."""
    x1, y1, x2, y2, a = corners(b)
    w = np.maximum(F32(0), np.minimum(x2[:, None], x2[None, :]) - np.maximum(x1[:, None], x1[None, :]))
    h = np.maximum(F32(0), np.minimum(y2[:, None], y2[None, :]) - np.maximum(y1[:, None], y1[None, :]))
    inter = w * h
    with np.errstate(invalid='ignore', divide='ignore'):
        o = inter / ((a[:, None] + a[None, :]) - inter)
    assert o.dtype == F32
    return o


def midpoint_distance(w64):
    """Relative distance of a float64 from the nearest midpoint of two neighbouring float32 values."""
    f = F32(w64)
    other = np.nextafter(f, F32(-np.inf) if np.float64(f) > w64 else F32(np.inf))
    mid = (np.float64(f) + np.float64(other)) / 2
    return abs(w64 - mid) / abs(w64)


def gaussian_weight(o, sigma, stats=None):
    o64 = np.float64(o)
    w64 = np.exp(-(o64 * o64) / np.float64(sigma))
    if stats is not None and o != 0:
        stats.weights += 1
        stats.midpoint = min(stats.midpoint, midpoint_distance(w64))
    return F32(w64)


def _hard(group, o, thr):
    """Greedy in order P.  group: positions in order P.  Returns the kept positions, in order P."""
    removed, kept = set(), []
    for a, i in enumerate(group):
        if i in removed:
            continue
        kept.append(i)
        for j in group[a + 1:]:
            if float(o[i, j]) > thr:
                removed.add(j)
    return kept


def _soft(group, o, t, idx, thr, gaussian, sigma, min_score, stats):
    """Soft-NMS of one group.  t: working scores (float32 array over positions, updated in place).  Returns the emitted
    positions in emission order; t holds each one's score at its pick."""
    left, out = list(group), []
    while left:
        best = left[0]
        for k in left[1:]:                                        # largest t; on a tie the lowest candidate index
            if t[k] > t[best] or (t[k] == t[best] and idx[k] < idx[best]):
                best = k
        if stats is not None and len(left) > 1:
            second = max(float(t[k]) for k in left if k != best)
            if second != float(t[best]) and t[best] != 0:
                stats.gap = min(stats.gap, (float(t[best]) - second) / abs(float(t[best])))
        if not t[best] >= F32(min_score):
            if stats is not None:
                stats.cut += 1
            break
        out.append(best)
        left.remove(best)
        for k in list(left):
            ok = o[best, k]
            if ok != ok:
                continue
            if gaussian:
                t[k] = t[k] * gaussian_weight(ok, sigma, stats)
            elif float(ok) > thr:
                t[k] = t[k] * (F32(1) - ok)
            if t[k] != t[k]:                                      # inf * 0: a box without a score is dropped
                left.remove(k)
    return out


def _merge_box(i, group, o, s, x1, y1, x2, y2, thr, stats):
    W = X1 = Y1 = X2 = Y2 = np.float64(0)
    n = 0
    for j in group:                                               # ascending position of P
        if j == i or float(o[i, j]) > thr:
            w = np.float64(s[j])
            W += w
            X1 += w * np.float64(x1[j]); Y1 += w * np.float64(y1[j]); X2 += w * np.float64(x2[j]); Y2 += w * np.float64(y2[j])
            n += 1
    if stats is not None and n > 1:
        stats.merged += 1
    a1, b1, a2, b2 = X1 / W, Y1 / W, X2 / W, Y2 / W
    return [F32((a1 + a2) * 0.5), F32((b1 + b2) * 0.5), F32(a2 - a1), F32(b2 - b1)]


def run(b, c, s, conf, thr, kind, agnostic=False, sigma=0.5, min_score=None, topk=512, stats=None):
    """One image.  b [N, 4 or 5], c [N] int64, s [N] float32.  See the module docstring for the result."""
    assert kind in KINDS
    b, c, s = np.asarray(b, F32), np.asarray(c, np.int64), np.asarray(s, F32)
    width = b.shape[1]
    if kind in ('soft-linear', 'soft-gaussian'):
        assert conf >= 0 and (min_score is None or min_score >= 0) and sigma > 0, 'MYDET_E_BADARG'
    if kind == 'merge':
        assert conf > 0, 'MYDET_E_BADARG'
        assert width == 4, 'MYDET_E_UNSUPP'
    min_score = F32(conf) if min_score is None else F32(min_score)
    empty = dict(index=np.zeros(0, np.int64), cls=np.zeros(0, np.int64), score=np.zeros(0, F32), bbox=np.zeros((0, width), F32))
    sel, bad = select(c, s, conf, topk)
    if bad:
        return dict(empty, count=-1)
    n = len(sel)
    sb, sc, ss = b[sel], c[sel], s[sel]                           # positions 0..n-1 are order P over all classes
    o = pair_matrix(sb)
    x1, y1, x2, y2, _ = corners(sb)
    groups = [list(range(n))] if agnostic else [list(np.nonzero(sc == k)[0]) for k in np.unique(sc)]
    groups = [g for g in groups if g]
    t = ss.copy()
    boxes = {}
    emitted = []                                                  # (group number, rank, position)
    for g, group in enumerate(groups):
        if kind in ('hard', 'merge'):
            order = _hard(group, o, thr)
            if kind == 'merge':
                for i in order:
                    boxes[i] = _merge_box(i, group, o, ss, x1, y1, x2, y2, thr, stats)
            if stats is not None and agnostic:
                kept = set(order)
                stats.cross_class += sum(1 for i in order for j in group if j not in kept and sc[i] != sc[j] and float(o[i, j]) > thr)
        else:
            order = _soft(group, o, t, sel, thr, kind == 'soft-gaussian', sigma, min_score, stats)
            if stats is not None:
                stats.reordered += order != sorted(order)
                if agnostic:
                    floor = 0.0 if kind == 'soft-gaussian' else thr
                    stats.cross_class += sum(1 for a, i in enumerate(order) for j in order[a + 1:] if sc[i] != sc[j] and float(o[i, j]) > floor)
        emitted += [(g, r, i) for r, i in enumerate(order)]
    # class ascending, and inside a class the order of selection (one group: its ranks; per-class groups: the class's own)
    emitted.sort(key=lambda e: (int(sc[e[2]]), e[0], e[1]))
    pos = np.asarray([i for _, _, i in emitted], np.int64)
    if len(pos) == 0:
        return dict(empty, count=0)
    bbox = sb[pos].copy()
    if kind == 'merge':
        bbox = np.asarray([boxes[i] for i in pos], F32).reshape(-1, 4)
    return dict(count=len(pos), index=sel[pos].astype(np.int64), cls=sc[pos], score=t[pos].astype(F32), bbox=bbox)
