"""The fused IoU-and-appearance cost of mydet_track_frames_appear_optimal_f32 restated (test code; the package never imports it).
Written from the rule text of include/mydet.h, not from the kernel: tests/_appear_ref.Stream (predict with the shift, update,
templates, retire, births, re-identification, sim and how) with the stage of tests/_assoc_ref.py -- a cost matrix, the
assignment of tests/_mot_ref.assign, optimal_gap -- on the fused integer cost:

    q = floor(iou * 65536), S = S(j, d) with the template before this frame's update, a = S >> 1
    eligible: as in mydet_track_assoc, and gate == 0 or has[j] == 0 or S >= gate
    m = q when has[j] == 0, else ((256 - weight) * q + weight * a) >> 8
    cost = 65536 - m when eligible, 131072 when not, 65536 on a dummy column

The IoUs are float64 here (as in _track_ref), so q may differ from the kernel's by a few units; the margins say when that cannot
matter: 'iou_thres', 'score', 'band' as in _assoc_ref, 'opt_gap' on the FUSED costs, `unchecked`, and _appear_ref's integer
'sim' margin to the gate and to reid.  `needed` is the workspace contract: {(d, j): S} of the last frame that was not a
bad-class frame."""
import numpy as np

import _appear_ref
import _assoc_ref
import _track_ref as ref
from _appear_ref import F, similarity
from _motion_ref import ShiftTrack

ONE, INELIGIBLE = _assoc_ref.ONE, _assoc_ref.INELIGIBLE


def affinity(q, S, has, weight):
    """m of one pair, in integers."""
    q, S, weight = int(q), int(S), int(weight)
    if not has:
        return q
    return ((256 - weight) * q + weight * (S >> 1)) >> 8


def cost_matrix(m, ok):
    """m int [n][mt] (the affinities), ok bool [n][mt] (eligible) -> int64 [n][mt + n]: the real columns, then one dummy per row."""
    n, mt = m.shape
    c = np.full((n, mt + n), ONE, np.int64)
    c[:, :mt] = np.where(ok, ONE - m.astype(np.int64), INELIGIBLE)
    return c


class Stream(_appear_ref.Stream):
    """_appear_ref.Stream with the optimal assignment on the fused cost in place of the walk."""

    def __init__(self, max_tracks, par, weight=0, **kw):
        super().__init__(max_tracks, par, **kw)
        assert 0 <= int(weight) <= 256
        self.weight = int(weight)
        self.margins.update(opt_gap=np.inf)
        self.unchecked = 0
        self.needed = {}

    def _stage(self, rows, iou, live, cats, desc, thr, second, match, how, stage):
        n, mt = len(rows), len(self.slots)
        m = np.zeros((n, mt), np.int64)
        ok = np.zeros((n, mt), bool)
        for i, d in enumerate(rows):
            for j, k in enumerate(live):
                t = self.slots[k]
                if t.cls != cats[d] or k in match or (second and t.missed != 1):
                    continue
                v = iou[d, j]
                if np.isnan(v):
                    continue
                self.margins['iou_thres'] = min(self.margins['iou_thres'], abs(v - thr))
                if not v > thr:
                    continue
                s = 0
                if self.has[k]:
                    s = similarity(self.tmpl[:, k], desc[d])
                    if self.gate > 0:
                        self.margins['sim'] = min(self.margins.get('sim', np.inf), abs(s - self.gate + 0.5))
                        if s < self.gate:
                            continue
                m[i, k], ok[i, k] = affinity(np.floor(v * 65536.0), s, self.has[k], self.weight), True
        cost = cost_matrix(m, ok)
        pairs, _ = _assoc_ref.optimal_pairs(cost, mt)
        gap, ties, unchecked = _assoc_ref.optimal_gap(cost, mt, pairs)
        self.margins['opt_gap'] = min(self.margins['opt_gap'], gap)
        self.ties += ties
        self.unchecked += unchecked
        for i, k in pairs:
            match[k] = int(rows[i])
            how[k] = stage

    def step(self, boxes, scores, cats, count, desc, shift=None):
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
            high = [d for d in order if scores[d] >= self.high]
            low = [d for d in order if self.low <= scores[d] < self.high]
        else:
            high, low = order, []
        live = [k for k, t in enumerate(self.slots) if t is not None]
        for k in live:
            self.slots[k].__class__ = ShiftTrack
            self.slots[k].predict(par)
        par.shift = None
        match, how, sim = {}, {}, {}
        self.needed = {}
        if live and n:
            iou = self._ious(boxes, [self.slots[k] for k in live])
            # the workspace contract: nothing here depends on the solver's outcome
            for band, thr, second in ((high, float(par.match_thres), False), (low, self.low_match if self.bands else 0.0, True)):
                for d in band:
                    for j, k in enumerate(live):
                        t = self.slots[k]
                        if not self.has[k] or t.cls != cats[d] or (second and t.missed != 1) or np.isnan(iou[d, j]):
                            continue
                        self.margins['iou_thres'] = min(self.margins['iou_thres'], abs(iou[d, j] - thr))
                        if iou[d, j] > thr:
                            self.needed[(d, k)] = similarity(self.tmpl[:, k], desc[d])
            if high:
                self._stage(high, iou, live, cats, desc, float(par.match_thres), False, match, how, 1)
            if low:
                self._stage(low, iou, live, cats, desc, self.low_match, True, match, how, 2)
        # re-identification: the rule text of mydet_track_frames_appear_f32, behind the solve
        if self.reid > 0:
            for d in high:
                if d in match.values() or not scores[d] >= new32:
                    continue
                best = None
                for k in live:
                    t = self.slots[k]
                    if k in match or t.cls != cats[d] or not self.has[k] or t.missed < 2:
                        continue
                    x = t.x.astype(np.float32)
                    lim = self.reach * F(max(x[2], x[3], boxes[d][2], boxes[d][3]))
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
        for d in high:
            if d in taken:
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


def run(frames, descs, width, img_hw, max_tracks, params=None, appear=None, assoc=None, shifts=None, weight=0, stream=None):
    """_appear_ref.run through a Stream of this module (a fresh one when None): (stream, outs, arrays)."""
    if stream is None:
        par = ref.Params(img_hw, np.float32, **(params or {}))
        stream = Stream(max_tracks, par, weight=weight, **(appear or {}), **(assoc or {}))
    return _appear_ref.run(frames, descs, width, img_hw, max_tracks, shifts=shifts, stream=stream)


def margins_hold(stream):
    """The margins every GPU case asserts on the restatement before it looks at the kernel: _assoc_ref's, on the fused costs,
    and the integer margin of every S that met the gate or reid (offset by a half: any value is decisive)."""
    m = stream.margins
    return bool(m['iou_thres'] >= 0.05 and m['score'] >= 1e-3 and m['band'] >= 1e-3 and m['opt_gap'] >= 0.05 * 65536 and
                stream.unchecked == 0 and stream.ties == 0 and m.get('sim', np.inf) > 0)
