"""Float64 numpy checker for rotated boxes (test code; the package never imports it).

Rows are (cx, cy, w, h, degrees); the angle is clockwise in image coordinates and the corners are those of the reference's
xywha2vertex (utils/bbox_ops.py:137-172): hori = (w/2 cos, w/2 sin), verti = (h/2 sin, -h/2 cos),
tl, tr, br, bl = c + verti - hori, c + verti + hori, c - verti + hori, c - verti - hori.

The IoU is the exact area of intersection: box b's corners are written in box a's orthonormal frame (origin at a's centre,
axes along hori and verti), where a is |u| <= w/2, |v| <= h/2, and clipped against its four sides (Sutherland-Hodgman,
vectorised over pairs).  `nms` is the greedy class-aware selection of the post-process kernel with the `>=` rule of the
reference's nms_rotbb (utils/bbox_ops.py:290).
"""
import numpy as np


def vertices(boxes):
    """[N,5] -> [N,4,2] float64: tl, tr, br, bl."""
    b = np.asarray(boxes, dtype=np.float64).reshape(-1, 5)
    rad = b[:, 4] * np.pi / 180.0
    c, s = np.cos(rad), np.sin(rad)
    hori = np.stack([b[:, 2] / 2 * c, b[:, 2] / 2 * s], axis=1)
    verti = np.stack([b[:, 3] / 2 * s, -b[:, 3] / 2 * c], axis=1)
    ctr = b[:, :2]
    return np.stack([ctr + verti - hori, ctr + verti + hori, ctr - verti + hori, ctr - verti - hori], axis=1)


def _clip(poly, n, axis, sign, bound):
    """Keep sign * poly[..., axis] <= bound.  poly [P,M,2], n [P] vertex counts -> ([P,2M,2], counts).  Every vertex is
    kept: a stage emits at most one vertex and one crossing point per input vertex, so 2M slots always hold the result
    (round-off at coincident edges can put near-boundary vertices alternately inside and outside, and the list then grows
    by more than the one vertex of the textbook case; the extra points are duplicates and carry no area)."""
    P, M, _ = poly.shape
    out = np.zeros((P, 2 * M, 2))
    cnt = np.zeros(P, dtype=np.int64)
    d = bound[:, None] - sign * poly[:, :, axis]
    rows = np.arange(P)
    for k in range(M):
        live = k < n
        k1 = np.where(k + 1 >= n, 0, min(k + 1, M - 1))
        cur, nxt = poly[:, k], poly[rows, k1]
        dc, dn = d[:, k], d[rows, k1]
        ina, inb = dc >= 0, dn >= 0
        r = rows[live & ina]
        out[r, cnt[r]] = cur[r]
        cnt[r] += 1
        r = rows[live & (ina != inb)]
        t = dc[r] / (dc[r] - dn[r])
        out[r, cnt[r]] = cur[r] + t[:, None] * (nxt[r] - cur[r])
        cnt[r] += 1
    return out[:, :max(int(cnt.max()), 1)], cnt


def iou_pairs(a, b):
    """IoU of a[p] with b[p]: [P,5], [P,5] -> [P] float64.  0 when the boxes do not overlap or one of them has no area;
    NaN only for 0/0 (both areas 0)."""
    a = np.asarray(a, dtype=np.float64).reshape(-1, 5)
    b = np.asarray(b, dtype=np.float64).reshape(-1, 5)
    P = a.shape[0]
    if P == 0:
        return np.zeros(0)
    rad = a[:, 4] * np.pi / 180.0
    c, s = np.cos(rad), np.sin(rad)
    rel = vertices(b) - a[:, None, :2]
    poly = np.stack([rel[:, :, 0] * c[:, None] + rel[:, :, 1] * s[:, None],
                     rel[:, :, 0] * s[:, None] - rel[:, :, 1] * c[:, None]], axis=2)
    n = np.full(P, 4, dtype=np.int64)
    hw, hh = np.abs(a[:, 2]) / 2, np.abs(a[:, 3]) / 2
    for axis, sign, bound in ((0, 1.0, hw), (0, -1.0, hw), (1, 1.0, hh), (1, -1.0, hh)):
        poly, n = _clip(poly, n, axis, sign, bound)
    M = poly.shape[1]
    twice = np.zeros(P)
    rows = np.arange(P)
    for k in range(M):
        k1 = np.where(k + 1 >= n, 0, min(k + 1, M - 1))
        nxt = poly[rows, k1]
        twice += np.where(k < n, poly[:, k, 0] * nxt[:, 1] - nxt[:, 0] * poly[:, k, 1], 0.0)
    area_a, area_b = a[:, 2] * a[:, 3], b[:, 2] * b[:, 3]
    inter = np.where((n >= 3) & (area_a != 0) & (area_b != 0), np.abs(twice) / 2, 0.0)
    with np.errstate(invalid='ignore', divide='ignore'):
        return inter / (area_a + area_b - inter)


def iou_matrix(a, b):
    """[N,5], [M,5] -> [N,M] float64."""
    a = np.asarray(a, dtype=np.float64).reshape(-1, 5)
    b = np.asarray(b, dtype=np.float64).reshape(-1, 5)
    ia, ib = np.meshgrid(np.arange(a.shape[0]), np.arange(b.shape[0]), indexing='ij')
    return iou_pairs(a[ia.ravel()], b[ib.ravel()]).reshape(a.shape[0], b.shape[0])


def aligned_iou_matrix(a, b):
    """Axis-aligned IoU of columns 0-3 (what the default post-process compares), float64."""
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    ax1, ay1, ax2, ay2 = a[:, 0] - a[:, 2] / 2, a[:, 1] - a[:, 3] / 2, a[:, 0] + a[:, 2] / 2, a[:, 1] + a[:, 3] / 2
    bx1, by1, bx2, by2 = b[:, 0] - b[:, 2] / 2, b[:, 1] - b[:, 3] / 2, b[:, 0] + b[:, 2] / 2, b[:, 1] + b[:, 3] / 2
    w = np.clip(np.minimum(ax2[:, None], bx2[None]) - np.maximum(ax1[:, None], bx1[None]), 0, None)
    h = np.clip(np.minimum(ay2[:, None], by2[None]) - np.maximum(ay1[:, None], by1[None]), 0, None)
    inter = w * h
    with np.errstate(invalid='ignore', divide='ignore'):
        return inter / ((a[:, 2] * a[:, 3])[:, None] + (b[:, 2] * b[:, 3])[None] - inter)


def select(cats, scores, conf, topk=512):
    """Candidate indices that pass `score >= conf` (float32), cut to the top-k by (score desc, index asc) and sorted by
    (class asc, score desc, index asc): the order in which the kernel runs the NMS."""
    scores = np.asarray(scores, dtype=np.float32)
    cats = np.asarray(cats)
    idx = np.nonzero(scores >= np.float32(conf))[0]
    idx = idx[np.lexsort((idx, -scores[idx].astype(np.float64)))][:topk]
    return idx[np.lexsort((idx, -scores[idx].astype(np.float64), cats[idx]))]


def same_class_ious(boxes, cats, order, iou=iou_matrix):
    """(IoU matrix of boxes[order], same-class mask) for the selected candidates."""
    m = iou(boxes[order], boxes[order])
    same = np.asarray(cats)[order][:, None] == np.asarray(cats)[order][None]
    return m, same


def nms(boxes, cats, scores, conf, nms_thres, topk=512, iou=iou_matrix, strict=False):
    """Greedy class-aware NMS: kept candidate indices in output order.  A box goes when its IoU with a kept box of its
    class, earlier in the order, is >= nms_thres (`strict`: > nms_thres, the axis-aligned kernel's rule)."""
    boxes = np.asarray(boxes)
    order = select(cats, scores, conf, topk)
    m, same = same_class_ious(boxes, cats, order, iou)
    with np.errstate(invalid='ignore'):
        sup = ((m > nms_thres) if strict else (m >= nms_thres)) & same
    kept = []
    for i in range(len(order)):
        if not any(sup[j, i] for j in kept):
            kept.append(i)
    return order[np.asarray(kept, dtype=np.int64)]


def margin(boxes, cats, order, nms_thres, iou=iou_matrix):
    """Smallest |IoU - nms_thres| over the same-class pairs of the selected candidates (NaN pairs ignored)."""
    m, same = same_class_ious(np.asarray(boxes), cats, order, iou)
    off = ~np.eye(len(order), dtype=bool)
    d = np.abs(m - nms_thres)[same & off]
    d = d[~np.isnan(d)]
    return d.min() if d.size else np.inf
