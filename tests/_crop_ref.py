"""The sampling rules of the object chips (include/mydet.h: mydet_crop_boxes_rgb) restated in numpy, from the header's text:
float32 scalars and arrays in the stated order for the coordinates, integers for the pixels.  For every chip value it gives
the value itself and the interval [lo, hi] the rules allow where a coordinate is not settled.

Settled.  The kernel's (c, s) are cosf / sinf of a float32 radian; this file takes float32 of the float64 cosine and sine.
A sub-sample is unsettled when the float64 value of (X - 0.5) * 32 + 0.5 or of (Y - 0.5) * 32 + 0.5, computed from the float64
cosine and sine, lies within 32 * TOL of an integer, TOL = 2e-4 px.  That is above what float32 can do to the formula
under the conditions `within_bound` checks (|X|, |Y| < 256, |lx|, |ly| <= 64, |angle| <= 360):
  * roundings.  sx, the offset (q + 0.5) / nx, two sums and the product give lx with 4 roundings and sx's relative 2^-24;
    lx*c, ly*s and the two sums of X add 4 more; every intermediate is below 256 in magnitude, where half an ulp is
    2^-17 = 7.6e-6 px: at most 13 such terms for X including ly's own, 1.0e-4 px.
  * cosine and sine.  The float32 radian r * (pi / 180) has a relative error of at most 2 * 2^-24 (the constant, the product),
    2 * pi * 1.2e-7 = 7.5e-7 in the angle; cosf / sinf are within 2 ulp, 1.2e-7.  |dc|, |ds| <= 8.7e-7 moves X by at most
    (|lx| + |ly|) * 8.7e-7 <= 128 * 8.7e-7 = 1.1e-4 px in the worst corner; the cases of tests/_crop_cases.py keep |lx|, |ly| <= 40
    in rotated boxes: 7e-5 px.
  * the quantiser.  X - 0.5 rounds once more (7.6e-6 px), * 32 is exact, + 0.5 rounds at a magnitude below 8192: half an
    ulp is 2^-11 / 2 of 1/32 px = 7.6e-6 px.
  Together below 1.0e-4 + 7e-5 + 1.6e-5 = 1.9e-4 < TOL.  An unsettled sub-sample contributes the minimum and the maximum of its
(at most four) neighbouring quantisations; lo and hi are the rounded means of those minima and maxima.  A settled chip value
has lo == hi, and the kernel must give exactly it."""
import math

import numpy as np

F = np.float32
TOL = 2e-4
MAX_Q = 2.0 ** 29


def valid_row(row):
    cx, cy, w, h, a = (float(v) for v in row)
    return all(math.isfinite(v) for v in (cx, cy, w, h, a)) and w > 0 and h > 0


def rotation(angle):
    """((c, s) float32, (c, s) float64) of an angle in degrees by the header's rule: 0 and the quarter turns exact."""
    a = float(F(angle))
    if a == 0.0:
        return (F(1), F(0)), (1.0, 0.0)
    r = math.fmod(a, 360.0)
    for deg, cs in (((90.0, -270.0), (0.0, 1.0)), ((180.0, -180.0), (-1.0, 0.0)), ((270.0, -90.0), (0.0, -1.0))):
        if r in deg:
            return (F(cs[0]), F(cs[1])), cs
    c, s = math.cos(math.radians(r)), math.sin(math.radians(r))
    return (F(c), F(s)), (c, s)


def _row5(row):
    row = np.asarray(row, dtype=np.float32).reshape(-1)
    return np.concatenate([row, np.zeros(5 - row.size, dtype=np.float32)]) if row.size == 4 else row


def _bilinear(img, fill, qx, qy):
    """The 8-bit bilinear values [..., 3] (int64) at the quantised points qx, qy (int64 arrays of one shape)."""
    H, W = img.shape[:2]
    x0, y0, fx, fy = qx >> 5, qy >> 5, (qx & 31)[..., None], (qy & 31)[..., None]

    def tap(y, x):
        inside = (y >= 0) & (y < H) & (x >= 0) & (x < W)
        v = img[np.clip(y, 0, H - 1), np.clip(x, 0, W - 1)].astype(np.int64)
        v[~inside] = fill
        return v
    top = tap(y0, x0) * (32 - fx) + tap(y0, x0 + 1) * fx
    bot = tap(y0 + 1, x0) * (32 - fx) + tap(y0 + 1, x0 + 1) * fx
    return (top * (32 - fy) + bot * fy + 512) >> 10


def geometry(row, size, pad):
    """What the coordinates of one chip are made of: dict with sx, sy, nx, ny (float32 rules) and the float32 and float64
    points X, Y of shape [ny, nx, ch, cw]."""
    ch, cw = size
    cx, cy, w, h, ang = (F(v) for v in _row5(row))
    (c, s), (c64, s64) = rotation(ang)
    pad = F(pad)
    with np.errstate(all='ignore'):
        sx, sy = (w * pad) / F(cw), (h * pad) / F(ch)
        nx, ny = (int(min(max(math.ceil(float(v)), 1), 4)) if math.isfinite(float(v)) else 4 for v in (sx, sy))
        i, j = np.arange(ch, dtype=F).reshape(1, 1, ch, 1), np.arange(cw, dtype=F).reshape(1, 1, 1, cw)
        offy = ((np.arange(ny, dtype=F) + F(0.5)) / F(ny)).reshape(ny, 1, 1, 1)
        offx = ((np.arange(nx, dtype=F) + F(0.5)) / F(nx)).reshape(1, nx, 1, 1)
        lx = (j + offx - F(0.5) * F(cw)) * sx
        ly = (i + offy - F(0.5) * F(ch)) * sy
        X = cx + lx * c - ly * s
        Y = cy + lx * s + ly * c
        assert X.dtype == np.float32 and Y.dtype == np.float32 and X.shape == (ny, nx, ch, cw)
        d = np.float64
        sx64, sy64 = d(w) * d(pad) / cw, d(h) * d(pad) / ch
        lx64 = (j.astype(d) + (np.arange(nx, dtype=d).reshape(1, nx, 1, 1) + 0.5) / nx - 0.5 * cw) * sx64
        ly64 = (i.astype(d) + (np.arange(ny, dtype=d).reshape(ny, 1, 1, 1) + 0.5) / ny - 0.5 * ch) * sy64
        X64 = d(cx) + lx64 * c64 - ly64 * s64
        Y64 = d(cy) + lx64 * s64 + ly64 * c64
    return dict(sx=sx, sy=sy, nx=nx, ny=ny, X=X, Y=Y, X64=X64, Y64=Y64, lx64=lx64, ly64=ly64)


def within_bound(row, size, pad):
    """The conditions under which TOL is derived (module docstring) hold for this chip."""
    g = geometry(row, size, pad)
    return bool(np.abs(g['X64']).max() < 256 and np.abs(g['Y64']).max() < 256 and np.abs(g['lx64']).max() <= 64
                and np.abs(g['ly64']).max() <= 64 and abs(float(_row5(row)[4])) <= 360)


def chip(img, row, size, pad=1.0, fill=(0, 0, 0)):
    """One chip of img uint8 [H, W, 3]: (value, lo, hi), uint8 [ch, cw, 3] each."""
    ch, cw = size
    fillv = np.asarray(fill, dtype=np.int64)
    if not valid_row(_row5(row)):
        v = np.broadcast_to(fillv.astype(np.uint8), (ch, cw, 3)).copy()
        return v, v.copy(), v.copy()
    g = geometry(row, size, pad)
    n = g['nx'] * g['ny']
    with np.errstate(all='ignore'):
        tx = np.floor((g['X'] - F(0.5)) * F(32) + F(0.5))
        ty = np.floor((g['Y'] - F(0.5)) * F(32) + F(0.5))
        assert tx.dtype == np.float32
        far = ~((np.abs(tx) <= MAX_Q) & (np.abs(ty) <= MAX_Q))          # NaN too: four fill taps
        qx, qy = np.where(far, 0, tx).astype(np.int64), np.where(far, 0, ty).astype(np.int64)
        val = _bilinear(img, fillv, qx, qy)
        val[far] = fillv
        vx, vy = (g['X64'] - 0.5) * 32 + 0.5, (g['Y64'] - 0.5) * 32 + 0.5
        vx, vy = np.where(far, 0.5, vx), np.where(far, 0.5, vy)
    kx, ky = np.rint(vx), np.rint(vy)
    ux, uy = np.abs(vx - kx) <= 32 * TOL, np.abs(vy - ky) <= 32 * TOL
    value = (val.sum(axis=(0, 1)) + (n >> 1)) // n
    if not (ux.any() or uy.any()):
        assert np.array_equal(qx, np.floor(vx).astype(np.int64)) and np.array_equal(qy, np.floor(vy).astype(np.int64))
        v = value.astype(np.uint8)
        return v, v.copy(), v.copy()
    xs = [np.where(ux, kx - 1, np.floor(vx)).astype(np.int64), np.where(ux, kx, np.floor(vx)).astype(np.int64)]
    ys = [np.where(uy, ky - 1, np.floor(vy)).astype(np.int64), np.where(uy, ky, np.floor(vy)).astype(np.int64)]
    assert ((qx == xs[0]) | (qx == xs[1])).all() and ((qy == ys[0]) | (qy == ys[1])).all(), 'float32 left the bound of TOL'
    alts = []
    for a in xs:
        for b in ys:
            v = _bilinear(img, fillv, a, b)
            v[far] = fillv
            alts.append(v)
    alts = np.stack(alts)
    lo = (alts.min(axis=0).sum(axis=(0, 1)) + (n >> 1)) // n
    hi = (alts.max(axis=0).sum(axis=(0, 1)) + (n >> 1)) // n
    assert (lo <= value).all() and (value <= hi).all()
    return value.astype(np.uint8), lo.astype(np.uint8), hi.astype(np.uint8)


def chips(frames, boxes, size, pad=1.0, fill=(0, 0, 0), counts=None, M=None):
    """(value, lo, hi, written): uint8 [B, M, ch, cw, 3] x 3 and bool [B, M]; slots that are not written hold zeros."""
    B, K = boxes.shape[:2]
    M = K if M is None else M
    out = [np.zeros((B, M) + tuple(size) + (3,), dtype=np.uint8) for _ in range(3)]
    written = np.zeros((B, M), dtype=bool)
    for b in range(B):
        n = min(K, M) if counts is None else min(int(counts[b]), K, M)
        for m in range(max(n, 0)):
            for o, v in zip(out, chip(frames[b], boxes[b, m], size, pad, fill)):
                o[b, m] = v
            written[b, m] = True
    return out[0], out[1], out[2], written


IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)


def to_float(chips_u8, norm):
    """uint8 [..., ch, cw, 3] -> float32 [..., 3, ch, cw]: x / 255, then with norm (x - mean) / std, in float32."""
    x = np.moveaxis(chips_u8, -1, -3).astype(np.float32) / F(255)
    if norm:
        mean = np.asarray(IMAGENET_MEAN, dtype=np.float32).reshape(3, 1, 1)
        std = np.asarray(IMAGENET_STD, dtype=np.float32).reshape(3, 1, 1)
        x = (x - mean) / std
    assert x.dtype == np.float32
    return x
