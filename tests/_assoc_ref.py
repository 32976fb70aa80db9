"""The associate step of mydet_track_frames_assoc_f32 in numpy: score bands and both assignments (test code; the package never
imports it).  Written from the rule text of include/mydet.h (mydet_track_assoc), not from the kernel.

`Stream` is tests/_track_ref.Stream with another `step`: predict, update, retire and births are the parent's Track methods and
the parent's order; only the association and the birth filter follow the new rules.  The optimal assignment is
tests/_mot_ref.assign on the cost matrix the rules define.  IoUs are float64 whatever the dtype (as in _track_ref); scores are
compared in float32, as the kernel compares them.

Margins, beside the parent's ('score': to min_score and new_thres):
  iou_thres   every IoU of a pair that is eligible but for its IoU, to its stage's threshold
  band        every score to low_thres and high_thres
  opt_gap     optimal only: the least total of a DIFFERENT pairing minus the optimal total.  The eligibility graph of a stage is
              cut into connected components and each component is enumerated exhaustively (every partial one-to-one map of its
              rows); a component too large for that counts in `unchecked`.  A gap of exactly 0 counts in `ties` instead.
"""
import numpy as np

import _mot_ref
import _track_ref as ref

ONE, INELIGIBLE = 65536, 131072
ENUM_ROWS = 7                                                        # a component's rows that are still enumerated


def cost_matrix(iou, ok):
    """iou [n][mt] float, ok [n][mt] bool (eligible but for the threshold test already applied by the caller) -> int64
    [n][mt + n]: the real columns, then one dummy per row."""
    n, mt = iou.shape
    c = np.full((n, mt + n), ONE, np.int64)
    q = np.floor(np.where(ok, iou, 0.0) * 65536.0).astype(np.int64)
    c[:, :mt] = np.where(ok, ONE - q, INELIGIBLE)
    return c


def optimal_pairs(cost, mt):
    """[(row, real column)] of the minimum-cost assignment, and its total."""
    col_of_row, total = _mot_ref.assign(cost)
    return [(r, c) for r, c in enumerate(col_of_row) if 0 <= c < mt and cost[r, c] != INELIGIBLE], total


def _components(ok):
    """Connected components of the bipartite eligibility graph: [(rows, columns)], rows with no eligible column left out."""
    n, mt = ok.shape
    seen_r, out = set(), []
    for r0 in range(n):
        if r0 in seen_r or not ok[r0].any():
            continue
        rows, cols, todo = {r0}, set(), [('r', r0)]
        while todo:
            kind, k = todo.pop()
            if kind == 'r':
                for c in np.flatnonzero(ok[k]):
                    if c not in cols:
                        cols.add(int(c))
                        todo.append(('c', int(c)))
            else:
                for r in np.flatnonzero(ok[:, k]):
                    if r not in rows:
                        rows.add(int(r))
                        todo.append(('r', int(r)))
        seen_r |= rows
        out.append((sorted(rows), sorted(cols)))
    return out


def _pairing_totals(cost, rows, cols):
    """{frozenset of (row, column): total} over every partial one-to-one map of `rows` into their eligible `cols`."""
    out = {}

    def walk(k, used, pairs, total):
        if k == len(rows):
            out[frozenset(pairs)] = total
            return
        r = rows[k]
        walk(k + 1, used, pairs, total + ONE)                        # the row's dummy
        for c in cols:
            if c not in used and cost[r, c] != INELIGIBLE:
                walk(k + 1, used | {c}, pairs + [(r, c)], total + int(cost[r, c]))
    walk(0, frozenset(), [], 0)
    return out


def optimal_gap(cost, mt, pairs):
    """(gap, ties, unchecked) of one solved stage: see the module docstring."""
    ok = cost[:, :mt] != INELIGIBLE
    gap, ties, unchecked = np.inf, 0, 0
    chosen = set(pairs)
    for rows, cols in _components(ok):
        if len(rows) > ENUM_ROWS:
            unchecked += 1
            continue
        totals = _pairing_totals(cost, rows, cols)
        mine = frozenset(p for p in chosen if p[0] in rows)
        best = totals[mine]
        assert best == min(totals.values()), 'the assignment is not optimal on a component'
        rest = [t for k, t in totals.items() if k != mine]
        if rest:
            g = min(rest) - best
            if g == 0:
                ties += 1
            else:
                gap = min(gap, g)
    return gap, ties, unchecked


class Stream(ref.Stream):
    def __init__(self, max_tracks, par, assign='greedy', low_thres=None, high_thres=None, low_match_thres=None):
        super().__init__(max_tracks, par)
        assert assign in ('greedy', 'optimal')
        self.assign, self.bands = assign, low_thres is not None
        if self.bands:
            assert high_thres is not None and low_match_thres is not None and np.float32(low_thres) < np.float32(high_thres)
            self.low, self.high, self.low_match = float(low_thres), float(high_thres), float(low_match_thres)
        self.margins.update(band=np.inf, opt_gap=np.inf)
        self.unchecked = 0

    def _stage(self, rows, iou, live, cats, thr, second, match):
        """Associate the detections `rows` (record slots in rank order) with the tracks not yet in `match`."""
        n, mt = len(rows), len(self.slots)
        full = np.zeros((n, mt))
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
                full[i, k], ok[i, k] = v, v > thr
        if self.assign == 'optimal':
            cost = cost_matrix(full, ok)
            pairs, _ = optimal_pairs(cost, mt)
            gap, ties, unchecked = optimal_gap(cost, mt, pairs)
            self.margins['opt_gap'] = min(self.margins['opt_gap'], gap)
            self.ties += ties
            self.unchecked += unchecked
            for i, k in pairs:
                match[k] = int(rows[i])
            return
        for i, d in enumerate(rows):
            cand = sorted(((full[i, k], k) for k in range(mt) if ok[i, k] and k not in match), key=lambda c: (-c[0], c[1]))
            if len(cand) > 1:
                gap = cand[0][0] - cand[1][0]
                if gap == 0:
                    self.ties += 1
                else:
                    self.margins['iou_gap'] = min(self.margins['iou_gap'], gap)
            if cand:
                match[cand[0][1]] = int(d)

    def step(self, boxes, scores, cats, count):
        par, mt = self.par, len(self.slots)
        if count < 0:
            return {'count': ref.BAD_CLASS, 'dropped': 0, 'id': [0] * mt, 'missed': [-1] * mt, 'match': [-1] * mt}
        n = min(int(count), 512)
        boxes = np.asarray(boxes, np.float32)[:n]
        if boxes.shape[1] == 4:
            boxes = np.concatenate([boxes, np.zeros((n, 1), np.float32)], axis=1)
        scores, cats = np.asarray(scores, np.float32)[:n], np.asarray(cats, np.int64)[:n]
        order = [int(d) for d in np.lexsort((np.arange(n), -scores.astype(np.float64)))]
        if self.bands:
            lo32, hi32 = np.float32(self.low), np.float32(self.high)
            for d in order:
                self.margins['band'] = min(self.margins['band'], abs(float(scores[d]) - self.low), abs(float(scores[d]) - self.high))
            high = [d for d in order if scores[d] >= hi32]
            low = [d for d in order if lo32 <= scores[d] < hi32]
        else:
            high, low = order, []
        live = [k for k, t in enumerate(self.slots) if t is not None]
        for k in live:
            self.slots[k].predict(par)
        match = {}                                                   # track slot -> record slot
        if live and n:
            iou = self._ious(boxes, [self.slots[k] for k in live])
            if high:
                self._stage(high, iou, live, cats, float(par.match_thres), False, match)
            if low:
                self._stage(low, iou, live, cats, self.low_match, True, match)
        for k, d in match.items():
            self.slots[k].update(boxes[d], scores[d], par)
        for k in live:
            t = self.slots[k]
            self.margins['score'] = min(self.margins['score'], abs(float(t.score) - float(par.min_score)))
            if not t.feasible(par) or t.missed >= par.max_missed:
                self.slots[k] = None
        taken = set(match.values())
        dropped, born = 0, {}
        for d in high:                                               # births: unmatched HIGH detections only
            if d in taken:
                continue
            self.margins['score'] = min(self.margins['score'], abs(float(scores[d]) - float(par.new_thres)))
            if not scores[d] >= np.float32(par.new_thres):
                continue
            free = [k for k, t in enumerate(self.slots) if t is None]
            if not free:
                dropped += 1
                continue
            self.slots[free[0]] = ref.Track(boxes[d], scores[d], cats[d], self.next_id, par)
            born[free[0]] = d
            self.next_id += 1
        return {'count': sum(t is not None for t in self.slots), 'dropped': dropped,
                'id': [t.id if t else 0 for t in self.slots], 'missed': [t.missed if t else -1 for t in self.slots],
                'match': [match.get(k, born.get(k, -1)) if t else -1 for k, t in enumerate(self.slots)]}


def run_case(case, dtype, img_hw):
    """A case of tests/_assoc_cases.py through a fresh Stream: (stream, the outputs of every frame)."""
    par = ref.Params(img_hw, dtype, match=case['match'], **case['params'])
    stream = Stream(case['max_tracks'], par, **case['assoc'])
    return stream, [stream.step(*ref.unpack_frame(r, case['width'])) for r in ref.pack_records(case['frames'], case['width'])]


def margins_hold(stream):
    """The margins every GPU case asserts on the float64 restatement before it looks at the kernel."""
    m = stream.margins
    return bool(m['iou_thres'] >= 0.05 and m['iou_gap'] >= 0.05 and m['score'] >= 1e-3 and m['band'] >= 1e-3 and
                m['opt_gap'] >= 0.05 * 65536 and stream.unchecked == 0)
