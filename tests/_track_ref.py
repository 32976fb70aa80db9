"""The whole tracker of include/mydet.h (mydet_track_frames_f32) in numpy, parameterised by dtype (test code; the package
never imports it).

In float64 it is the checker: tests/test_track_host.py holds its filter to the reference's KFTracklet on
tests/golden/kf_tracklet.npz.  In float32 it is the kernel's operation order written down -- every line below is one rounded
operation of csrc/track.hip (built with -ffp-contract=off), so the state must agree bit for bit.  The association compares IoUs
in float64 whatever the dtype (tests/_rotbox_ref.py); the test fixtures keep every decision away from its threshold and
`Stream.margins` records by how much.

The 10 x 10 covariance of the reference's RotBBoxKalmanFilter is five 2 x 2 blocks: parameter i couples only with its own
velocity, so a track is x[5], v[5], pxx[5], pxv[5], pvv[5], a score and the count of predictions since the last update."""
import numpy as np

import _rotbox_ref as chk

# KFTracklet's constants (reference utils/structures.py:457-460): standard deviations
P0 = (0.1, 0.1, 0.1, 0.1, 10, 0.1, 0.1, 0.1, 0.1, 10)
Q = (0.049, 0.032, 0.052, 0.097, 13.62, 0.01, 0.01, 0.01, 0.01, 1)
R = (0.073, 0.064, 0.124, 0.163, 24.39)
BAD_CLASS = -1


class Params:
    def __init__(self, img_hw, dtype=np.float32, match='iou', match_thres=0.3, new_thres=0.3, max_missed=30, momentum=0.8,
                 min_score=0.1, p0=P0, q=Q, r=R):
        dt = self.dtype = np.dtype(dtype).type
        # variances: squared in double, rounded once (ops.track_variances)
        self.p0, self.q, self.r = (np.square(np.asarray(v, np.float64)).astype(dt) for v in (p0, q, r))
        self.momentum, self.min_score = dt(np.float32(momentum)), dt(np.float32(min_score))
        self.new_thres, self.match_thres = dt(np.float32(new_thres)), dt(np.float32(match_thres))
        if dt is np.float64:                                         # the checker works with the exact decimal constants
            self.momentum, self.min_score, self.new_thres, self.match_thres = (dt(v) for v in (momentum, min_score, new_thres, match_thres))
        self.max_missed, self.match = int(max_missed), match
        self.img_h, self.img_w = dt(img_hw[0]), dt(img_hw[1])


def mod180(a):
    """Python's a % 180 in a's own precision."""
    return np.remainder(a, type(a)(180))


class Track:
    def __init__(self, z, score, cls, tid, par):
        """RotBBoxKalmanFilter.initiate after KFTracklet.__init__'s angle % 180."""
        dt = par.dtype
        self.x = np.array(z, dtype=dt)
        self.x[4] = mod180(self.x[4])
        area = self.x[2] * self.x[3]
        self.v = np.zeros(5, dt)
        self.pxx, self.pvv = par.p0[:5].copy(), par.p0[5:].copy()
        self.pxx[:4] = par.p0[:4] * area
        self.pvv[:4] = par.p0[5:9] * area
        self.pxv = np.zeros(5, dt)
        self.score, self.missed, self.cls, self.id = dt(score), 0, int(cls), int(tid)
        self.box = self.x.copy()

    def predict(self, par):
        area = self.x[2] * self.x[3]
        qx, qv = par.q[:5].copy(), par.q[5:].copy()
        qx[:4] = par.q[:4] * area
        qv[:4] = par.q[5:9] * area
        t = self.pxv + self.pvv
        self.pxx = ((self.pxx + self.pxv) + t) + qx
        self.pxv = t
        self.pvv = self.pvv + qv
        self.x = self.x + self.v
        self.box = self.x.copy()                                     # what KFTracklet.predict returns: the angle not yet reduced
        self.x[4] = mod180(self.x[4])
        if self.missed >= 1:
            self.score = par.momentum * self.score
        self.missed += 1

    def update(self, z, det_score, par):
        dt = par.dtype
        z = np.array(z, dtype=dt)
        za = mod180(z[4])
        best, dmin = za, abs(za - self.x[4])
        for c in (za - dt(180), za + dt(180)):
            d = abs(c - self.x[4])
            if d < dmin:
                best, dmin = c, d
        z[4] = best
        area = self.x[2] * self.x[3]
        rr = par.r.copy()
        rr[:4] = par.r[:4] * area
        y = z - self.x
        inv = dt(1) / (self.pxx + rr)
        kx, kv = self.pxx * inv, self.pxv * inv
        self.x = self.x + kx * y
        self.v = self.v + kv * y
        oxx, oxv = self.pxx, self.pxv
        self.pxx = oxx - kx * oxx
        self.pxv = oxv - kx * oxv
        self.pvv = self.pvv - kv * oxv
        self.box = self.x.copy()                                     # what KFTracklet.update returns
        self.x[4] = mod180(self.x[4])
        self.score = par.momentum * self.score + (dt(1) - par.momentum) * dt(det_score)
        self.missed = 0

    def feasible(self, par):
        x = self.x
        if self.score < par.min_score or (x[:4] < 0).any():
            return False
        return not (x[0] > par.img_w or x[1] > par.img_h or x[2] > par.img_w or x[3] > par.img_h)


class Stream:
    """One stream of the tracker: `slots` (Track or None), the id counter, and the smallest margins of every decision taken."""

    def __init__(self, max_tracks, par):
        self.par, self.slots, self.next_id = par, [None] * max_tracks, 1
        self.margins = {'iou_thres': np.inf, 'iou_gap': np.inf, 'score': np.inf}
        self.ties = 0

    def _ious(self, boxes, tracks):
        tb = np.array([t.x for t in tracks], np.float64).reshape(-1, 5)
        db = np.asarray(boxes, np.float64).reshape(-1, 5)
        if self.par.match == 'rotated':
            return chk.iou_matrix(db, tb)
        return chk.aligned_iou_matrix(db[:, :4], tb[:, :4])

    def step(self, boxes, scores, cats, count):
        """One frame: boxes [512, 4 or 5] float32, scores [512] float32, cats [512] int64, `count` valid.  Returns the frame's
        outputs as a dict (per slot: id, cls, missed, matched record slot or -1; live count; dropped)."""
        par, mt = self.par, len(self.slots)
        if count < 0:
            return {'count': BAD_CLASS, 'dropped': 0, 'id': [0] * mt, 'missed': [-1] * mt, 'match': [-1] * mt}
        n = min(int(count), 512)
        boxes = np.asarray(boxes, np.float32)[:n]
        if boxes.shape[1] == 4:
            boxes = np.concatenate([boxes, np.zeros((n, 1), np.float32)], axis=1)
        scores, cats = np.asarray(scores, np.float32)[:n], np.asarray(cats, np.int64)[:n]
        order = np.lexsort((np.arange(n), -scores.astype(np.float64)))
        live = [k for k, t in enumerate(self.slots) if t is not None]
        for k in live:
            self.slots[k].predict(par)
        match = {}                                                   # track slot -> record slot
        if live and n:
            iou = self._ious(boxes, [self.slots[k] for k in live])
            thr = float(par.match_thres)
            for d in order:
                cand = [(iou[d, j], k) for j, k in enumerate(live) if self.slots[k].cls == cats[d]]
                for v, _ in cand:
                    if not np.isnan(v):
                        self.margins['iou_thres'] = min(self.margins['iou_thres'], abs(v - thr))
                cand = sorted(((v, k) for v, k in cand if k not in match and v > thr), key=lambda c: (-c[0], c[1]))
                if len(cand) > 1:
                    gap = cand[0][0] - cand[1][0]
                    if gap == 0:
                        self.ties += 1
                    else:
                        self.margins['iou_gap'] = min(self.margins['iou_gap'], gap)
                if cand:
                    match[cand[0][1]] = int(d)
        for k, d in match.items():
            self.slots[k].update(boxes[d], scores[d], par)
        for k in live:
            t = self.slots[k]
            self.margins['score'] = min(self.margins['score'], abs(float(t.score) - float(par.min_score)))
            if not t.feasible(par) or t.missed >= par.max_missed:
                self.slots[k] = None
        taken = set(match.values())
        dropped = 0
        born = {}
        for d in order:
            if int(d) in taken:
                continue
            self.margins['score'] = min(self.margins['score'], abs(float(scores[d]) - float(par.new_thres)))
            if not scores[d] >= np.float32(par.new_thres):
                continue
            free = [k for k, t in enumerate(self.slots) if t is None]
            if not free:
                dropped += 1
                continue
            self.slots[free[0]] = Track(boxes[d], scores[d], cats[d], self.next_id, par)
            born[free[0]] = int(d)
            self.next_id += 1
        out = {'count': sum(t is not None for t in self.slots), 'dropped': dropped,
               'id': [t.id if t else 0 for t in self.slots], 'missed': [t.missed if t else -1 for t in self.slots],
               'match': [match.get(k, born.get(k, -1)) if t else -1 for k, t in enumerate(self.slots)]}
        return out

    def arrays(self):
        """The state as ops.track_state_views names it: x, v, pxx, pxv, pvv [5, MT], score, cls, id, missed [MT]; free slots 0."""
        mt, dt = len(self.slots), self.par.dtype
        out = {k: np.zeros((5, mt), dt) for k in ('x', 'v', 'pxx', 'pxv', 'pvv')}
        out.update(score=np.zeros(mt, dt), cls=np.zeros(mt, np.int64), id=np.zeros(mt, np.int64), missed=np.zeros(mt, np.int32))
        for k, t in enumerate(self.slots):
            if t is not None:
                for name in ('x', 'v', 'pxx', 'pxv', 'pvv'):
                    out[name][:, k] = getattr(t, name)
                out['score'][k], out['cls'][k], out['id'][k], out['missed'][k] = t.score, t.cls, t.id, t.missed
        return out


def pack_records(frames, width):
    """[(boxes [n, width], scores [n], cats [n]) or None (a bad-class frame)] -> int32 [len(frames), words] wire records
    (include/mydet.h MYDET_REC_*; the INDEX plane is left zero)."""
    words = 4100 + (512 if width == 5 else 0)
    rec = np.zeros((len(frames), words), np.int32)
    for i, fr in enumerate(frames):
        if fr is None:
            rec[i, 0] = BAD_CLASS
            continue
        b, s, c = (np.asarray(a) for a in fr)
        n = len(s)
        rec[i, 0] = n
        if n == 0:
            continue
        b = b.astype(np.float32).reshape(n, -1)
        rec[i, 4:4 + 4 * n] = np.ascontiguousarray(b[:, :4]).view(np.int32).reshape(-1)
        rec[i, 2052:2052 + n] = s.astype(np.float32).view(np.int32)
        rec[i, 2564:2564 + 2 * n] = c.astype(np.int64).view(np.int32)
        if width == 5:
            rec[i, 4100:4100 + n] = np.ascontiguousarray(b[:, 4]).view(np.int32)
    return rec


def unpack_frame(rec_row, width):
    """One wire record -> (boxes [512, width], scores [512], cats [512], count)."""
    r = np.asarray(rec_row, np.int32)
    b = r[4:2052].view(np.float32).reshape(512, 4)
    if width == 5:
        b = np.concatenate([b, r[4100:4612].view(np.float32)[:, None]], axis=1)
    return b, r[2052:2564].view(np.float32), r[2564:3588].view(np.int64), int(r[0])
