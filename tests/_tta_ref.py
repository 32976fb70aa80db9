"""Numpy restatement of test-time augmentation (test code; the package never imports it): the mirrored frame, the view
transform of the boxes, the fusion of view records by NMS -- through tests/_tiles_ref.py and tests/_nms_ref.py, which already
restate the merge -- and Weighted Boxes Fusion by the rules of include/mydet.h (mydet_fuse_view_records_f32), in float32 and
float64 in the stated order, so that the kernel's output is compared with `==`.

    fields of one frame: boxes [V,512,4|5] float32 in the pixel coordinates of the mirrored frame, scores [V,512], cats [V,512],
    counts [V]; flips [V] of MYDET_VIEW_* bits; frame_hw = (H, W).
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _nms_ref as nref  # noqa: E402
import _tiles_ref as tref  # noqa: E402

F32, F64 = np.float32, np.float64
HFLIP, VFLIP = 1, 2
TOPK = 512
VIEWS_MAX = 8


def flip_frame(a, flip, rows_axis=-3):
    """The mirrored view of frames whose rows are axis `rows_axis` and columns the next one ([...,H,W,3] by default)."""
    a = np.asarray(a)
    rows_axis %= a.ndim
    if flip & VFLIP:
        a = np.flip(a, rows_axis)
    if flip & HFLIP:
        a = np.flip(a, rows_axis + 1)
    return np.ascontiguousarray(a)


def view_transform(boxes, flips, frame_hw):
    """The boxes of every view back in frame coordinates: cx' = (float)W - cx (HFLIP), cy' = (float)H - cy (VFLIP), one float32
    subtraction each; angle' = -angle when exactly one bit is set, not wrapped.  [V,512,4|5] -> a float32 copy."""
    out = np.array(boxes, dtype=F32)
    H, W = F32(frame_hw[0]), F32(frame_hw[1])
    for v, f in enumerate(flips):
        if f & HFLIP:
            out[v, :, 0] = W - out[v, :, 0]
        if f & VFLIP:
            out[v, :, 1] = H - out[v, :, 1]
        if out.shape[2] == 5 and f in (HFLIP, VFLIP):
            out[v, :, 4] = -out[v, :, 4]
    return out


def nms_record(boxes, scores, cats, counts, flips, frame_hw, thres, metric='iou', rotated_nms=False):
    """MYDET_FUSE_NMS, class-aware: the merge of tile records on the transformed boxes with all origins zero (int32 words)."""
    V = len(flips)
    return tref.expected_record(view_transform(boxes, flips, frame_hw), scores, cats, counts, [(0, 0)] * V, thres, metric, rotated_nms)


def nms_margin(boxes, scores, cats, counts, flips, frame_hw, thres, metric='iou', rotated_nms=False):
    """Smallest distance of a same-class pair value of the selected candidates from the threshold (the checker is float64)."""
    V = len(flips)
    kept, cb, cc, cs, order = tref.merge_frame(view_transform(boxes, flips, frame_hw), scores, cats, counts, [(0, 0)] * V, thres, metric,
                                               rotated_nms)
    return np.inf if kept is None else tref.margin(cb, cc, order, thres, metric, rotated_nms)


def nms_agnostic_record(boxes, scores, cats, counts, flips, frame_hw, thres):
    """MYDET_FUSE_NMS with agnostic (metric 'iou'): hard NMS with one group on the candidates, conf = -inf (tests/_nms_ref.py)."""
    V = len(flips)
    cb, cc, cs = tref.candidates(view_transform(boxes, flips, frame_hw), scores, cats, counts, [(0, 0)] * V)
    width = cb.shape[1]
    ob, os_, oc, oi = np.zeros((TOPK, width), F32), np.zeros(TOPK, F32), np.zeros(TOPK, np.int64), np.zeros(TOPK, np.int32)
    if any(int(c) == tref.BAD_CLASS for c in counts):
        return tref.pack_record(ob, os_, oc, tref.BAD_CLASS, oi)
    out = nref.run(cb, cc, cs, -np.inf, thres, 'hard', agnostic=True)
    k = out['count']
    ob[:k], os_[:k], oc[:k], oi[:k] = out['bbox'], out['score'], out['cls'], out['index']
    return tref.pack_record(ob, os_, oc, k, oi)


def _corners(cx, cy, w, h):
    """x1, y1, x2, y2, area of (arrays of) float32 rows in the kernel's operation order."""
    hw, hh = w / F32(2), h / F32(2)
    x1, y1, x2, y2 = cx - hw, cy - hh, cx + hw, cy + hh
    return x1, y1, x2, y2, (x2 - x1) * (y2 - y1)


def _iou(a, b):
    """float32 IoU of corner tuples (arrays broadcast): inter / (area_a + area_b - inter); 0/0 is NaN."""
    ww = np.maximum(F32(0), np.minimum(a[2], b[2]) - np.maximum(a[0], b[0]))
    hh = np.maximum(F32(0), np.minimum(a[3], b[3]) - np.maximum(a[1], b[1]))
    inter = ww * hh
    with np.errstate(invalid='ignore', divide='ignore'):
        o = inter / ((a[4] + b[4]) - inter)
    assert np.asarray(o).dtype == F32
    return o


def wbf_frame(boxes, scores, cats, counts, flips, frame_hw, thres, agnostic=False, min_score=0.0, stats=None):
    """MYDET_FUSE_WBF of one frame: dict(count, bbox [K,4] float32, score [K] float32, cls [K] int64, index [K]); count -1 for a
    frame with a bad-class view.  stats: an optional dict that receives 'clusters' (before the min_score cut), 'dropped' (candidates
    the 512-cluster cap dropped), 'joined' (candidates that joined an existing cluster) and 'late' (joins after the cap was met)."""
    V = len(flips)
    assert 1 <= V <= VIEWS_MAX and np.asarray(boxes).shape[2] == 4
    empty = dict(bbox=np.zeros((0, 4), F32), score=np.zeros(0, F32), cls=np.zeros(0, np.int64), index=np.zeros(0, np.int64))
    if any(int(c) == tref.BAD_CLASS for c in counts):
        return dict(empty, count=-1)
    cb, cc, cs = tref.candidates(view_transform(boxes, flips, frame_hw), scores, cats, counts, [(0, 0)] * V)
    with np.errstate(invalid='ignore'):
        live = np.nonzero(cs > F32(0))[0]                         # NaN (past a view's count), zeros and negatives are skipped
    if ((cc[live] < 0) | (cc[live] > 4095)).any():
        return dict(empty, count=-1)
    order = live[np.argsort(-(cs[live] + F32(0)), kind='stable')]  # order P: score descending, candidate index ascending
    x1, y1, x2, y2, area = _corners(cb[:, 0], cb[:, 1], cb[:, 2], cb[:, 3])
    S = np.zeros((TOPK, 5), F64)                                  # Wt, X1, Y1, X2, Y2
    Fr = np.zeros((TOPK, 4), F32)                                 # the fused rows
    n, cls, first = np.zeros(TOPK, np.int64), np.zeros(TOPK, np.int64), np.zeros(TOPK, np.int64)
    ncl = dropped = joined = late = 0
    for c in order:
        j = -1
        if ncl:
            o = _iou(_corners(Fr[:ncl, 0], Fr[:ncl, 1], Fr[:ncl, 2], Fr[:ncl, 3]), (x1[c], y1[c], x2[c], y2[c], area[c]))
            with np.errstate(invalid='ignore'):
                ok = o.astype(F64) > thres                        # a NaN never matches
            if not agnostic:
                ok &= cls[:ncl] == cc[c]
            if ok.any():
                best = o[ok].max()
                j = int(np.nonzero(ok & (o == best))[0][0])       # a tie goes to the lowest j
        if j < 0:
            if ncl == TOPK:
                dropped += 1
                continue
            j, ncl = ncl, ncl + 1
            cls[j], first[j] = cc[c], c
        else:
            joined += 1
            late += ncl == TOPK
        w = F64(cs[c])
        S[j] += np.array([w, w * F64(x1[c]), w * F64(y1[c]), w * F64(x2[c]), w * F64(y2[c])], F64)
        n[j] += 1
        a1, b1, a2, b2 = S[j, 1] / S[j, 0], S[j, 2] / S[j, 0], S[j, 3] / S[j, 0], S[j, 4] / S[j, 0]
        Fr[j] = [F32((a1 + a2) * 0.5), F32((b1 + b2) * 0.5), F32(a2 - a1), F32(b2 - b1)]
    if stats is not None:
        stats.update(clusters=ncl, dropped=dropped, joined=joined, late=late)
    f = ((S[:ncl, 0] / n[:ncl].astype(F64)) * (np.minimum(n[:ncl], V).astype(F64) / F64(V))).astype(F32)
    keep = np.nonzero(~(f < F32(min_score)))[0]
    keep = keep[np.lexsort((keep, -(f[keep] + F32(0)), cls[keep]))]        # class ascending, f descending, creation order
    return dict(count=len(keep), bbox=Fr[keep], score=f[keep], cls=cls[keep], index=first[keep])


def wbf_record(*args, **kwargs):
    """wbf_frame as the int32 words of a record: slots past the count zero."""
    out = wbf_frame(*args, **kwargs)
    ob, os_, oc, oi = np.zeros((TOPK, 4), F32), np.zeros(TOPK, F32), np.zeros(TOPK, np.int64), np.zeros(TOPK, np.int32)
    k = max(out['count'], 0)
    ob[:k], os_[:k], oc[:k], oi[:k] = out['bbox'], out['score'], out['cls'], out['index']
    return tref.pack_record(ob, os_, oc, out['count'], oi)


def view_plan(scales, hflip, vflip):
    """The views of Augment(hflip, vflip, scales): the cross product of the scales with '', 'h', 'v', 'hv', in that order."""
    flips = [0] + ([HFLIP] if hflip else []) + ([VFLIP] if vflip else []) + ([HFLIP | VFLIP] if hflip and vflip else [])
    return [(float(s), f) for s in scales for f in flips]


def view_input_size(input_size, scale, div):
    return input_size if scale == 1.0 else max(div, int(round(input_size * scale / div)) * div)
