"""The appearance rules of include/mydet.h restated (test code; the package never imports it): the descriptor of
mydet_appear_boxes_rgb_u8 in numpy -- float32 in the stated order for the coordinates, integers for the rest -- and the tracker
of mydet_track_frames_appear_f32 in plain Python over the arithmetic of tests/_track_ref.py.

Settled.  The kernel's (c, s) are cosf / sinf of a float32 radian; this file takes float32 of the float64 cosine and sine (as
tests/_crop_ref.py).  At angle 0 and at the quarter turns (c, s) are exact and every float32 operation here is the kernel's, so
the descriptors must be equal whatever the coordinates.  At any other angle a sample is UNSETTLED when its float64 X or Y,
computed from the float64 cosine and sine, lies within TOL = 2e-4 px of an integer.  That is above what float32 can do to the
formula under the conditions `within_bound` checks (|X|, |Y| < 256, |lx|, |ly| <= 40, |angle| <= 360):
  * roundings.  w * 0.75f rounds once (/ 16 and / 32 are exact), the sample offset (j + 0.5 - 8) is exact, lx rounds once;
    lx*c, ly*s and the two sums of X add 4 more; every intermediate is below 256 in magnitude, where half an ulp is
    2^-17 = 7.6e-6 px: at most 9 such terms for X including ly's own, 6.9e-5 px.
  * cosine and sine.  As derived in _crop_ref.py: |dc|, |ds| <= 8.7e-7 moves X by at most (|lx| + |ly|) * 8.7e-7 <= 80 * 8.7e-7 = 7e-5 px.
  Together below 1.4e-4 < TOL (there is no quantiser here: the pixel is floorf(X)).  An unsettled sample may fall into either of
its (at most four) neighbouring pixels."""
import math

import numpy as np

import _track_ref as ref
from _crop_ref import TOL, _row5, rotation
from _motion_ref import ShiftTrack

F = np.float32
BINS, ROWS, COLS, SAMPLES, SIM_MAX = 128, 32, 16, 512, 131072
MAX_XY = 2.0 ** 29


def quarter(angle):
    """The angle is 0 or a quarter turn: (c, s) are exact."""
    a = float(F(angle))
    return a == 0.0 or math.fmod(a, 360.0) in (90.0, -270.0, 180.0, -180.0, 270.0, -90.0)


def geometry(row):
    """The sample points of one box: dict with the float32 X, Y [32, 16] and their float64 counterparts (lx64, ly64 too)."""
    cx, cy, w, h, ang = (F(v) for v in _row5(row))
    with np.errstate(all='ignore'):
        if math.isfinite(float(ang)):
            (c, s), (c64, s64) = rotation(ang)
        else:
            (c, s), (c64, s64) = (F(np.nan), F(np.nan)), (math.nan, math.nan)
        sx, sy = w * F(0.75) / F(16), h * F(0.75) / F(32)
        i, j = np.arange(ROWS, dtype=F).reshape(ROWS, 1), np.arange(COLS, dtype=F).reshape(1, COLS)
        lx = (j + F(0.5) - F(8)) * sx
        ly = (i + F(0.5) - F(16)) * sy
        X = cx + lx * c - ly * s
        Y = cy + lx * s + ly * c
        assert X.dtype == np.float32 and Y.dtype == np.float32 and X.shape == (ROWS, COLS)
        d = np.float64
        lx64 = (j.astype(d) + 0.5 - 8.0) * (d(w) * 0.75 / 16) + np.zeros((ROWS, COLS))
        ly64 = (i.astype(d) + 0.5 - 16.0) * (d(h) * 0.75 / 32) + np.zeros((ROWS, COLS))
        X64 = d(cx) + lx64 * c64 - ly64 * s64
        Y64 = d(cy) + lx64 * s64 + ly64 * c64
    return dict(X=X, Y=Y, X64=X64, Y64=Y64, lx64=lx64, ly64=ly64)


def within_bound(row):
    """The conditions under which TOL is derived (module docstring) hold for this box."""
    g = geometry(row)
    with np.errstate(all='ignore'):
        return bool(np.abs(g['X64']).max() < 256 and np.abs(g['Y64']).max() < 256 and np.abs(g['lx64']).max() <= 40
                    and np.abs(g['ly64']).max() <= 40 and abs(float(_row5(row)[4])) <= 360)


def _bins(img, half, y, x):
    px = img[y, x].astype(np.int64)
    return half * 64 + (px[..., 0] >> 6) * 16 + (px[..., 1] >> 6) * 4 + (px[..., 2] >> 6)


def describe(img, row):
    """One box on img uint8 [H, W, 3]: dict with desc (uint16 [128], the restatement's own descriptor), settled (int64 [128],
    the histogram of the settled samples), u (the number of unsettled samples) and reach (bool [128], the bins an unsettled
    sample can fall into)."""
    H, W = img.shape[:2]
    g = geometry(row)
    X, Y = g['X'], g['Y']
    with np.errstate(all='ignore'):
        counted = (np.abs(X) <= F(MAX_XY)) & (np.abs(Y) <= F(MAX_XY))                 # false for a NaN
        fx, fy = np.floor(np.where(counted, X, 0)).astype(np.int64), np.floor(np.where(counted, Y, 0)).astype(np.int64)
    x, y = np.clip(fx, 0, W - 1), np.clip(fy, 0, H - 1)
    half = (np.arange(ROWS).reshape(ROWS, 1) >> 4) + np.zeros((ROWS, COLS), np.int64)
    bins = _bins(img, half, y, x)
    desc = np.bincount(bins[counted], minlength=BINS).astype(np.uint16)
    if quarter(_row5(row)[4]) or not counted.any():
        return dict(desc=desc, settled=desc.astype(np.int64), u=0, reach=np.zeros(BINS, bool))
    assert counted.all(), 'a rotated box of the cases is finite'
    X64, Y64 = g['X64'], g['Y64']
    kx, ky = np.rint(X64), np.rint(Y64)
    ux, uy = np.abs(X64 - kx) <= TOL, np.abs(Y64 - ky) <= TOL
    uns = ux | uy
    xs = [np.where(ux, kx - 1, np.floor(X64)).astype(np.int64), np.where(ux, kx, np.floor(X64)).astype(np.int64)]
    ys = [np.where(uy, ky - 1, np.floor(Y64)).astype(np.int64), np.where(uy, ky, np.floor(Y64)).astype(np.int64)]
    assert ((fx == xs[0]) | (fx == xs[1])).all() and ((fy == ys[0]) | (fy == ys[1])).all(), 'float32 left the bound of TOL'
    reach = np.zeros(BINS, bool)
    for a in xs:
        for b in ys:
            reach[_bins(img, half, np.clip(b, 0, H - 1), np.clip(a, 0, W - 1))[uns]] = True
    settled = np.bincount(bins[~uns], minlength=BINS).astype(np.int64)
    return dict(desc=desc, settled=settled, u=int(uns.sum()), reach=reach)


def descriptors(frames, boxes, counts=None):
    """(desc uint16 [B, K, 128], info [B][K] -- the describe() dicts, None for a row that is not a box) of frames uint8
    [B, H, W, 3] and boxes float32 [B, K, 4 | 5]; rows at or beyond the count (a negative count is 0) are zeros."""
    B, K = boxes.shape[:2]
    desc = np.zeros((B, K, BINS), np.uint16)
    info = [[None] * K for _ in range(B)]
    for b in range(B):
        n = K if counts is None else max(0, min(int(counts[b]), K))
        for k in range(n):
            info[b][k] = describe(frames[b], boxes[b, k])
            desc[b, k] = info[b][k]['desc']
    return desc, info


# ---- the tracker with the appearance ----

def level(v):
    """A fraction of the largest similarity on the scale of S (ops.appear_set): floor(v * 131072 + 0.5); None is 0."""
    return 0 if v is None else int(math.floor(float(v) * SIM_MAX + 0.5))


def alpha_of(momentum):
    return int(math.floor((1.0 - float(momentum)) * 256 + 0.5))


def blend(t, d, alpha):
    """One template bin: t += ((256*d - t) * alpha) >> 8 with an arithmetic shift (Python's >> floors, as the kernel's does)."""
    return int(t) + (((256 * int(d) - int(t)) * int(alpha)) >> 8)


def similarity(tmpl, d):
    """S = sum of min(tmpl[b], 256 * d[b]) in integers."""
    return int(np.minimum(np.asarray(tmpl, np.int64), 256 * np.asarray(d, np.int64)).sum())


class Stream(ref.Stream):
    """tests/_track_ref.Stream with the greedy association of mydet_track_assoc (one band or two), the shift of
    mydet_track_frames_motion_f32 and the appearance rules: gate, re-identification, templates, sim and how.  has [MT] and
    tmpl [128][MT] are the appearance state.  Margins beside the parent's: 'band', and 'sim' -- every S that was compared, to
    gate or reid (integers: any margin > 0 is decisive)."""

    def __init__(self, max_tracks, par, gate=0, reid=0, alpha=26, reach=2.0, update_thres=0.3, low_thres=None, high_thres=None,
                 low_match_thres=None):
        super().__init__(max_tracks, par)
        self.gate, self.reid, self.alpha, self.reach, self.update_thres = int(gate), int(reid), int(alpha), F(reach), F(update_thres)
        self.bands = low_thres is not None
        if self.bands:
            self.low, self.high, self.low_match = F(low_thres), F(high_thres), float(F(low_match_thres))
        self.has = np.zeros(max_tracks, np.int32)
        self.tmpl = np.zeros((BINS, max_tracks), np.int32)
        self.margins.update(band=np.inf)

    def _take(self, k, d):
        """The template of slot k follows descriptor d (a match above update_thres)."""
        if self.has[k]:
            self.tmpl[:, k] = [blend(t, v, self.alpha) for t, v in zip(self.tmpl[:, k], d)]
        else:
            self.tmpl[:, k] = 256 * d.astype(np.int32)
            self.has[k] = 1

    def step(self, boxes, scores, cats, count, desc, shift=None):
        """One frame; desc uint16 [512, 128], row = record slot.  The parent's outputs, and sim, how per slot."""
        par, mt = self.par, len(self.slots)
        if count < 0:
            return {'count': ref.BAD_CLASS, 'dropped': 0, 'id': [0] * mt, 'missed': [-1] * mt, 'match': [-1] * mt,
                    'sim': [-1] * mt, 'how': [-1] * mt}
        par.shift = None if shift is None or int(shift[2]) != 1 else (int(shift[0]), int(shift[1]))
        n = min(int(count), 512)
        boxes = np.asarray(boxes, np.float32)[:n]
        if boxes.shape[1] == 4:
            boxes = np.concatenate([boxes, np.zeros((n, 1), np.float32)], axis=1)
        scores, cats = np.asarray(scores, np.float32)[:n], np.asarray(cats, np.int64)[:n]
        desc = np.asarray(desc)
        order = [int(d) for d in np.lexsort((np.arange(n), -scores.astype(np.float64)))]
        new32 = F(par.new_thres)
        if self.bands:
            for d in order:
                self.margins['band'] = min(self.margins['band'], abs(float(scores[d]) - float(self.low)), abs(float(scores[d]) - float(self.high)))
            stage = {d: 1 if scores[d] >= self.high else 2 if self.low <= scores[d] < self.high else 0 for d in order}
        else:
            stage = {d: 1 for d in order}
        live = [k for k, t in enumerate(self.slots) if t is not None]
        for k in live:
            self.slots[k].__class__ = ShiftTrack
            self.slots[k].predict(par)
        par.shift = None
        match, how, sim = {}, {}, {}
        # 1. the walk, with the gate
        if live and n:
            iou = self._ious(boxes, [self.slots[k] for k in live])
            for d in order:
                if stage[d] == 0:
                    continue
                thr = float(par.match_thres) if stage[d] == 1 else self.low_match
                cand = []
                for j, k in enumerate(live):
                    t = self.slots[k]
                    if t.cls != cats[d] or k in match or (stage[d] == 2 and t.missed != 1):
                        continue
                    v = iou[d, j]
                    if np.isnan(v):
                        continue
                    self.margins['iou_thres'] = min(self.margins['iou_thres'], abs(v - thr))
                    if not v > thr:
                        continue
                    if self.gate > 0 and self.has[k]:
                        s = similarity(self.tmpl[:, k], desc[d])
                        self.margins['sim'] = min(self.margins.get('sim', np.inf), abs(s - self.gate + 0.5))
                        if s < self.gate:
                            continue
                    cand.append((v, k))
                cand.sort(key=lambda c: (-c[0], c[1]))
                if len(cand) > 1:
                    gap = cand[0][0] - cand[1][0]
                    if gap == 0:
                        self.ties += 1
                    else:
                        self.margins['iou_gap'] = min(self.margins['iou_gap'], gap)
                if cand:
                    match[cand[0][1]] = d
                    how[cand[0][1]] = stage[d]
        # 2. re-identification
        if self.reid > 0:
            for d in order:
                if d in match.values() or stage[d] != 1 or not scores[d] >= new32:
                    continue
                best = None
                for k in live:
                    t = self.slots[k]
                    if k in match or t.cls != cats[d] or not self.has[k] or t.missed < 2:
                        continue
                    x = t.x.astype(np.float32)
                    m = max(x[2], x[3], boxes[d][2], boxes[d][3])
                    lim = self.reach * F(m)
                    assert lim.dtype == np.float32
                    if not (abs(boxes[d][0] - x[0]) <= lim and abs(boxes[d][1] - x[1]) <= lim):
                        continue
                    s = similarity(self.tmpl[:, k], desc[d])
                    self.margins['sim'] = min(self.margins.get('sim', np.inf), abs(s - self.reid + 0.5))
                    if s >= self.reid and (best is None or s > best[0]):
                        best = (s, k)
                if best is not None:
                    match[best[1]] = d
                    how[best[1]] = 3
        # 3. update, templates
        for k, d in match.items():
            sim[k] = similarity(self.tmpl[:, k], desc[d])
            self.slots[k].update(boxes[d], scores[d], par)
            if scores[d] >= self.update_thres:
                self._take(k, desc[d])
        for k in live:
            t = self.slots[k]
            self.margins['score'] = min(self.margins['score'], abs(float(t.score) - float(par.min_score)))
            if not t.feasible(par) or t.missed >= par.max_missed:
                self.slots[k] = None
                self.has[k] = 0
                self.tmpl[:, k] = 0
        taken = set(match.values())
        dropped, born = 0, {}
        for d in order:
            if d in taken or stage[d] != 1:
                continue
            self.margins['score'] = min(self.margins['score'], abs(float(scores[d]) - float(par.new_thres)))
            if not scores[d] >= new32:
                continue
            free = [k for k, t in enumerate(self.slots) if t is None]
            if not free:
                dropped += 1
                continue
            k = free[0]
            self.slots[k] = ref.Track(boxes[d], scores[d], cats[d], self.next_id, par)
            self.tmpl[:, k] = 256 * desc[d].astype(np.int32)
            self.has[k] = 1
            born[k] = d
            self.next_id += 1
        out = {'count': sum(t is not None for t in self.slots), 'dropped': dropped,
               'id': [t.id if t else 0 for t in self.slots], 'missed': [t.missed if t else -1 for t in self.slots],
               'match': [match.get(k, born.get(k, -1)) if t else -1 for k, t in enumerate(self.slots)]}
        out['how'] = [-1 if t is None else 4 if k in born else how.get(k, 0) for k, t in enumerate(self.slots)]
        out['sim'] = [sim[k] if t is not None and k in sim and k not in born else -1 for k, t in enumerate(self.slots)]
        return out


def run(frames, descs, width, img_hw, max_tracks, params=None, appear=None, assoc=None, shifts=None, stream=None):
    """frames (for _track_ref.pack_records) and descs uint16 [F, 512, 128] through a Stream (a fresh one when None):
    (stream, the outputs of every frame, the state arrays after every frame -- the parent's, and has, tmpl)."""
    if stream is None:
        par = ref.Params(img_hw, np.float32, **(params or {}))
        stream = Stream(max_tracks, par, **(appear or {}), **(assoc or {}))
    outs, arrays = [], []
    for f, r in enumerate(ref.pack_records(frames, width)):
        outs.append(stream.step(*ref.unpack_frame(r, width), descs[f], shift=None if shifts is None else shifts[f]))
        a = stream.arrays()
        a.update(has=stream.has.copy(), tmpl=stream.tmpl.copy())
        arrays.append(a)
    return stream, outs, arrays
