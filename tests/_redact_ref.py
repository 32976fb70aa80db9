"""Numpy restatement of the redaction rules (include/mydet.h: mydet_redact_boxes_*), written from the rules and not
from the kernel: float64 geometry, everything else integers.  The colour of 'solid' in 4:2:0 comes from the documented host
function ops.rgb_to_yuv, which tests/test_draw_host.py checks on its own."""
import math

import numpy as np

from mydetection_amd import ops

EPS = 1e-3          # a pixel whose coverage by a row changes when (a, b) move by +-EPS is "unsettled" for float32 (as in _draw_ref)


def _ab(H, W, row):
    cx, cy, _, _, ang = (float(v) for v in row)
    c, s = (1.0, 0.0) if ang == 0 else (math.cos(math.radians(ang)), math.sin(math.radians(ang)))
    dx = (np.arange(W, dtype=np.float64) + 0.5 - cx)[None, :]
    dy = (np.arange(H, dtype=np.float64) + 0.5 - cy)[:, None]
    return np.abs(dx * c + dy * s), np.abs(-dx * s + dy * c)


def _covers(a, b, ra, rb, shape):
    if shape == 'box':
        return (a <= ra) & (b <= rb)
    return (a * rb) ** 2 + (b * ra) ** 2 <= (ra * rb) ** 2


def valid_row(row):
    return bool(np.all(np.isfinite(np.asarray(row, dtype=np.float64))) and row[2] > 0 and row[3] > 0)


def _rows(boxes):
    boxes = np.asarray(boxes, dtype=np.float64)
    if boxes.shape[1] == 4:
        boxes = np.concatenate([boxes, np.zeros((boxes.shape[0], 1))], axis=1)
    return boxes


def coverage(H, W, boxes, count, style, classes=None):
    """(covered, unsettled) masks [H, W] of one frame's list under an ops.RedactStyle.  A pixel is unsettled when the coverage
    by some row changes as (a, b) move by +-EPS and no row covers it beyond doubt.  An axis-aligned 'box' row (angle 0, values
    at multiples of 1/8, pad 1.0 or 1.25) is exact in float32 and unsettles nothing."""
    boxes = _rows(boxes)
    K = boxes.shape[0]
    covered, shaky, firm = (np.zeros((H, W), dtype=bool) for _ in range(3))
    count = K if count is None else min(int(count), K)
    for k in range(max(count, 0)):
        row = boxes[k]
        if not valid_row(row):
            continue
        if style.classes is not None and int(classes[k]) not in style.classes:
            continue
        a, b = _ab(H, W, row)
        ra, rb = float(row[2]) / 2 * style.pad, float(row[3]) / 2 * style.pad
        cov = _covers(a, b, ra, rb, style.shape)
        uns = np.zeros((H, W), dtype=bool)
        if not (float(row[4]) == 0 and style.shape == 'box'):
            for da in (-EPS, EPS):
                for db in (-EPS, EPS):
                    uns |= _covers(np.maximum(a + da, 0), np.maximum(b + db, 0), ra, rb, style.shape) != cov
        covered |= cov
        shaky |= uns
        firm |= cov & ~uns
    return covered, shaky & ~firm


def cell_means(plane, cc):
    """int64 [nI, nJ]: (2*S + n) // (2*n) per cell of cc x cc samples anchored at the origin, n the samples inside the plane."""
    H, W = plane.shape
    nI, nJ = -(-H // cc), -(-W // cc)
    full = np.zeros((nI * cc, nJ * cc), dtype=np.int64)
    ones = np.zeros_like(full)
    full[:H, :W] = plane
    ones[:H, :W] = 1
    S = full.reshape(nI, cc, nJ, cc).sum(axis=(1, 3))
    n = ones.reshape(nI, cc, nJ, cc).sum(axis=(1, 3))
    return (2 * S + n) // (2 * n)


def mosaic(plane, cc):
    H, W = plane.shape
    M = cell_means(plane, cc)
    return M[(np.arange(H) // cc)[:, None], (np.arange(W) // cc)[None, :]]


def smooth(plane, cc):
    H, W = plane.shape
    M = cell_means(plane, cc)
    nI, nJ = M.shape

    def taps(n, cells):
        u = 2 * np.arange(n, dtype=np.int64) + 1 - cc
        k0 = np.floor_divide(u, 2 * cc)
        return u - 2 * cc * k0, np.clip(k0, 0, cells - 1), np.clip(k0 + 1, 0, cells - 1)

    fy, Ia, Ib = (v[:, None] for v in taps(H, nI))
    fx, Ja, Jb = (v[None, :] for v in taps(W, nJ))
    t = 2 * cc
    top = (t - fx) * M[Ia, Ja] + fx * M[Ia, Jb]
    bot = (t - fx) * M[Ib, Ja] + fx * M[Ib, Jb]
    return ((t - fy) * top + fy * bot + 2 * cc * cc) // (4 * cc * cc)


def new_plane(plane, cc, style, color):
    """What every sample of `plane` becomes where it is redacted (int64 [H, W]); cc: the cell size on this plane's grid."""
    p = plane.astype(np.int64)
    if style.mode == 'solid':
        return np.full(p.shape, int(color), dtype=np.int64)
    return mosaic(p, cc) if style.mode == 'mosaic' else smooth(p, cc)


def redact_rgb(img, boxes, count, style, classes=None):
    """Redact one frame [H, W, 3] uint8 in place; returns the unsettled-pixel mask [H, W]."""
    H, W, _ = img.shape
    covered, unsettled = coverage(H, W, boxes, count, style, classes)
    if covered.any():
        new = [new_plane(img[..., c], style.cell, style, style.color[c]) for c in range(3)]
        for c in range(3):
            img[..., c][covered] = new[c][covered].astype(np.uint8)
    return unsettled


def quads(mask, H2, W2):
    """[H2, 2, W2, 2] view of a luma mask with the frame's odd edge padded by False."""
    H, W = mask.shape
    m = np.zeros((2 * H2, 2 * W2), dtype=bool)
    m[:H, :W] = mask
    return m.reshape(H2, 2, W2, 2)


def redact_yuv(Y, U, V, boxes, count, style, matrix='bt601', full_range=False, classes=None):
    """Redact one 4:2:0 frame in place: Y [H, W], U and V [ceil(H/2), ceil(W/2)] uint8; returns (unsettled luma mask, unsettled
    chroma mask): a chroma sample is unsettled if its quad holds an unsettled pixel and no settled covered one."""
    H, W = Y.shape
    H2, W2 = U.shape
    covered, unsettled = coverage(H, W, boxes, count, style, classes)
    cq = quads(covered, H2, W2).any(axis=(1, 3))
    uq = quads(unsettled, H2, W2).any(axis=(1, 3)) & ~quads(covered & ~unsettled, H2, W2).any(axis=(1, 3))
    if covered.any():
        col = [int(v) for v in ops.rgb_to_yuv(np.asarray(style.color, dtype=np.uint8), matrix, full_range)]
        ny = new_plane(Y, style.cell, style, col[0])
        nu, nv = new_plane(U, style.cell // 2, style, col[1]), new_plane(V, style.cell // 2, style, col[2])
        Y[covered] = ny[covered].astype(np.uint8)
        U[cq], V[cq] = nu[cq].astype(np.uint8), nv[cq].astype(np.uint8)
    return unsettled, uq
