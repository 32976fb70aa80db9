"""Numpy restatement of the merge of tile records (test code; the package never imports it).

The records of T windows of one frame become T*512 candidates -- candidate t*512 + k is slot k of window t with the window's
origin added to its centre in float32; slots past a window's count carry a NaN score -- and the frame's record is what the
post-process gives on them with conf_thres = -inf: selection and greedy class-aware NMS by tests/_rotbox_ref.py (float64
pair values), with the axis-aligned IoU or the intersection over the smaller area and `>`, or the rotated IoU and `>=`.
Also the record buffer layout (MYDET_REC_* of include/mydet.h) in numpy, to pack test inputs and unpack results.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _rotbox_ref as chk  # noqa: E402

TOPK = 512
REC_COUNT, REC_BBOX = 0, 4
REC_SCORE = REC_BBOX + 4 * TOPK
REC_CLASS = REC_SCORE + TOPK
REC_INDEX = REC_CLASS + 2 * TOPK
REC_WORDS = REC_INDEX + TOPK
REC_ROT_WORDS = REC_WORDS + TOPK
BAD_CLASS = -1


def ios_matrix(a, b):
    """Intersection over the smaller area of columns 0-3 (cx, cy, w, h), float64: [N,4+], [M,4+] -> [N,M]; NaN for 0/0."""
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    ax1, ay1, ax2, ay2 = a[:, 0] - a[:, 2] / 2, a[:, 1] - a[:, 3] / 2, a[:, 0] + a[:, 2] / 2, a[:, 1] + a[:, 3] / 2
    bx1, by1, bx2, by2 = b[:, 0] - b[:, 2] / 2, b[:, 1] - b[:, 3] / 2, b[:, 0] + b[:, 2] / 2, b[:, 1] + b[:, 3] / 2
    w = np.clip(np.minimum(ax2[:, None], bx2[None]) - np.maximum(ax1[:, None], bx1[None]), 0, None)
    h = np.clip(np.minimum(ay2[:, None], by2[None]) - np.maximum(ay1[:, None], by1[None]), 0, None)
    with np.errstate(invalid='ignore', divide='ignore'):
        return (w * h) / np.minimum((a[:, 2] * a[:, 3])[:, None], (b[:, 2] * b[:, 3])[None])


def pair_rule(metric, rotated_nms):
    """(pair-value matrix function, strict) of a merge: strict = suppress at value > threshold, else >=."""
    if rotated_nms:
        assert metric == 'iou'
        return chk.iou_matrix, False
    return {'iou': chk.aligned_iou_matrix, 'ios': ios_matrix}[metric], True


def candidates(boxes, scores, cats, counts, origins):
    """The candidate arrays of one frame.  boxes [T,512,4|5] float32 in window coordinates, scores [T,512], cats [T,512],
    counts [T], origins [T] pairs (x0, y0) -> (boxes [T*512, 4|5] float32, cats [T*512], scores [T*512] float32)."""
    boxes = np.array(boxes, dtype=np.float32)
    scores = np.array(scores, dtype=np.float32)
    T = boxes.shape[0]
    for t, (x0, y0) in enumerate(origins):
        boxes[t, :, 0] = boxes[t, :, 0] + np.float32(x0)              # one float32 add each
        boxes[t, :, 1] = boxes[t, :, 1] + np.float32(y0)
        scores[t, max(int(counts[t]), 0):] = np.nan
    return boxes.reshape(T * TOPK, -1), np.asarray(cats).reshape(T * TOPK), scores.reshape(T * TOPK)


def merge_frame(boxes, scores, cats, counts, origins, nms_thres, metric='iou', rotated_nms=False):
    """(kept candidate indices in output order or None for a frame with a bad-class window, candidate boxes, cats, scores,
    selection order) of one frame."""
    cb, cc, cs = candidates(boxes, scores, cats, counts, origins)
    if any(int(c) == BAD_CLASS for c in counts):
        return None, cb, cc, cs, None
    iou, strict = pair_rule(metric, rotated_nms)
    order = chk.select(cc, cs, -np.inf)
    kept = chk.nms(cb, cc, cs, -np.inf, nms_thres, iou=iou, strict=strict)
    return kept, cb, cc, cs, order


def margin(cb, cc, order, nms_thres, metric='iou', rotated_nms=False):
    """Smallest |pair value - nms_thres| over the same-class pairs of the selected candidates."""
    return chk.margin(cb, cc, order, nms_thres, iou=pair_rule(metric, rotated_nms)[0])


def pack_record(boxes, scores, cats, count, index=None):
    """One record (int32 words) from its fields: boxes [512,4] or [512,5] (the fifth column goes to the angle plane)."""
    boxes = np.asarray(boxes, dtype=np.float32)
    rot = boxes.shape[1] == 5
    r = np.zeros(REC_ROT_WORDS if rot else REC_WORDS, np.int32)
    r[REC_COUNT] = count
    r[REC_BBOX:REC_SCORE] = np.ascontiguousarray(boxes[:, :4]).view(np.int32).ravel()
    r[REC_SCORE:REC_CLASS] = np.asarray(scores, dtype=np.float32).view(np.int32)
    r[REC_CLASS:REC_INDEX] = np.asarray(cats, dtype=np.int64).view(np.int32)
    if index is not None:
        r[REC_INDEX:REC_WORDS] = index
    if rot:
        r[REC_WORDS:REC_ROT_WORDS] = np.ascontiguousarray(boxes[:, 4]).view(np.int32)
    return r


def unpack_records(rec):
    """Fields of a record buffer [..., words] int32 as numpy arrays: count, bbox [...,512,4], score, class_idx, index(, angle)."""
    rec = np.ascontiguousarray(rec)
    lead = rec.shape[:-1]
    out = {'count': rec[..., REC_COUNT],
           'pad': rec[..., 1:REC_BBOX],
           'bbox': np.ascontiguousarray(rec[..., REC_BBOX:REC_SCORE]).view(np.float32).reshape(lead + (TOPK, 4)),
           'score': np.ascontiguousarray(rec[..., REC_SCORE:REC_CLASS]).view(np.float32),
           'class_idx': np.ascontiguousarray(rec[..., REC_CLASS:REC_INDEX]).view(np.int64),
           'index': rec[..., REC_INDEX:REC_WORDS]}
    if rec.shape[-1] == REC_ROT_WORDS:
        out['angle'] = np.ascontiguousarray(rec[..., REC_WORDS:REC_ROT_WORDS]).view(np.float32)
    return out


def expected_record(boxes, scores, cats, counts, origins, nms_thres, metric='iou', rotated_nms=False):
    """The merged record of one frame as int32 words, by the rules above."""
    kept, cb, cc, cs, _ = merge_frame(boxes, scores, cats, counts, origins, nms_thres, metric, rotated_nms)
    width = cb.shape[1]
    ob, os_, oc, oi = np.zeros((TOPK, width), np.float32), np.zeros(TOPK, np.float32), np.zeros(TOPK, np.int64), np.zeros(TOPK, np.int32)
    if kept is None:
        return pack_record(ob, os_, oc, BAD_CLASS, oi)
    k = len(kept)
    ob[:k], os_[:k], oc[:k], oi[:k] = cb[kept], cs[kept], cc[kept], kept
    return pack_record(ob, os_, oc, k, oi)
