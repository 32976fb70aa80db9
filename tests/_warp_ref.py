"""The similarity model of the camera-motion estimator (include/mydet.h: mydet_motion_warp_frames_rgb_u8) in Python integers,
and the tracker's predict step with a warp row (mydet_track_frames_warp_f32) in numpy float32, on top of tests/_motion_ref.py,
tests/_track_ref.py and tests/_assoc_ref.py (test code; the package never imports it).  Written from the rule text, not from the
kernels: sorts where the kernel ranks by counting, Python's unbounded integers with the int64 bound of the header asserted."""
import math

import numpy as np

import _assoc_ref
import _motion_ref as mref
import _track_ref

ONE = 1 << 16
T_LIMIT = 1 << 24                                                    # Q16: a fitted translation of 256 pixels or more is no result
U_MAX = 1 << 14                                                      # the domain of the arctangent polynomial: |u| <= 1/4
ATAN_C = (961263669, 320421223, 192252734, 137323381)                # round(180 / pi / (1, 3, 5, 7) * 2^24)
DEFAULT_TOL_Q, DEFAULT_ZOOM_Q, DEFAULT_ROT_Q = 2 * ONE, ONE // 8, 7 * ONE


def q16(v):
    """A real setting as the Q16 integer the settings struct carries."""
    return int(round(float(v) * ONE))


class Fit:
    """The settings of the fit, Q16: tolerance (pixels), max_zoom (|s - 1|), max_rotation (degrees)."""

    def __init__(self, tolerance=2.0, max_zoom=None, max_rotation=None):
        self.tol_q = q16(tolerance)
        self.zoom_q = DEFAULT_ZOOM_Q if max_zoom is None else q16(max_zoom)
        self.rot_q = DEFAULT_ROT_Q if max_rotation is None else q16(max_rotation)
        assert 0 < self.tol_q <= 16 * ONE and 0 < self.zoom_q <= ONE // 4 and 0 < self.rot_q <= 14 * ONE


def i64(v):
    """v, after the check that the device's int64 holds it."""
    assert -(1 << 63) <= v < (1 << 63), 'an intermediate of the fit leaves int64'
    return v


def isqrt(v):
    """floor(sqrt(v)) of v >= 0, bit by bit."""
    r, bit = 0, 1 << 62
    while bit > v:
        bit >>= 2
    while bit:
        if v >= r + bit:
            v -= r + bit
            r = (r >> 1) + bit
        else:
            r >>= 1
        bit >>= 2
    return r


def atan_deg_q(u):
    """Q16 degrees of atan(u / 2^16) for |u| <= U_MAX: the odd polynomial u (c1 - u2 (c3 - u2 (c5 - u2 c7))) on |u|, u2 = u^2 in
    Q16, the constants in Q24, every shift a floor on non-negative values."""
    m = abs(u)
    assert m <= U_MAX
    u2 = (m * m) >> 16
    p = ATAN_C[3]
    for c in ATAN_C[2::-1]:
        p = c - ((u2 * p) >> 16)
    d = (m * p) >> 24
    return -d if u < 0 else d


def derived(a, b, fit):
    """(s_q, deg_q) of a model, or None where a cap or the polynomial's domain is left."""
    s_q = isqrt(i64((ONE + a) ** 2 + b * b))
    if abs(s_q - ONE) > fit.zoom_q or ONE + a <= 0:
        return None
    u = i64(b << 16) // (ONE + a)
    if abs(u) > U_MAX:
        return None
    deg_q = atan_deg_q(u)
    if abs(deg_q) > fit.rot_q:
        return None
    return s_q, deg_q


def model_parts(a, b, qx, qy):
    """(M - I)(p - c) in Q16 pixels for p - c = (qx, qy) / 2: the floor of the half."""
    return i64(a * qx - b * qy) >> 1, i64(b * qx + a * qy) >> 1


def fit_model(g, blocks, valid, fit):
    """The fit over the valid blocks (ascending block indices `valid`): (a, b, tx, ty, s_q, deg_q, n_inliers, inlier block
    indices), or None for an invalid frame."""
    k, n = g.k, len(valid)
    ux, uy = [b % g.nbx for b in valid], [b // g.nbx for b in valid]
    px, py = [(g.R + 16 * u + 8) * k for u in ux], [(g.R + 16 * u + 8) * k for u in uy]
    qx, qy = [2 * p - g.W for p in px], [2 * p - g.H for p in py]   # p - c in half pixels
    dx, dy = [int(blocks[b, 4]) for b in valid], [int(blocks[b, 5]) for b in valid]
    h = n // 2
    if h == 0:
        return None                                                  # no pair
    al, bl = [], []
    for i in range(h):
        j = i + (n - h)
        ex, ey, fx, fy = px[j] - px[i], py[j] - py[i], dx[j] - dx[i], dy[j] - dy[i]
        den = ex * ex + ey * ey
        assert den > 0                                               # two blocks never share a centre
        al.append(i64((ex * fx + ey * fy) << 16) // den)
        bl.append(i64((ex * fy - ey * fx) << 16) // den)
    a, b = mref.lower_median(al), mref.lower_median(bl)
    parts = [model_parts(a, b, qx[i], qy[i]) for i in range(n)]
    tx = mref.lower_median([(dx[i] << 16) - parts[i][0] for i in range(n)])
    ty = mref.lower_median([(dy[i] << 16) - parts[i][1] for i in range(n)])
    inl = []
    for _ in range(2):
        inl = []
        for i in range(n):
            mx, my = model_parts(a, b, qx[i], qy[i])
            if abs((dx[i] << 16) - tx - mx) <= fit.tol_q and abs((dy[i] << 16) - ty - my) <= fit.tol_q:
                inl.append(i)
        m = len(inl)
        if m < 3:
            return None
        sux, suy, sdx, sdy = (sum(v[i] for i in inl) for v in (ux, uy, dx, dy))
        suu = sum(ux[i] * ux[i] + uy[i] * uy[i] for i in inl)
        sud = sum(ux[i] * dx[i] + uy[i] * dy[i] for i in inl)
        sxd = sum(ux[i] * dy[i] - uy[i] * dx[i] for i in inl)
        den = i64(16 * k * (m * suu - (sux * sux + suy * suy)))
        if den == 0:
            return None                                              # unreachable with three distinct blocks; the rule names it
        a = i64((m * sud - (sux * sdx + suy * sdy)) << 16) // den
        b = i64((m * sxd - (sux * sdy - suy * sdx)) << 16) // den
        sqx, sqy = sum(qx[i] for i in inl), sum(qy[i] for i in inl)
        tx = i64((sdx << 17) - (a * sqx - b * sqy)) // (2 * m)
        ty = i64((sdy << 17) - (b * sqx + a * sqy)) // (2 * m)
    d = derived(a, b, fit)
    if d is None or abs(tx) >= T_LIMIT or abs(ty) >= T_LIMIT:
        return None
    assert all(-(1 << 31) <= v < (1 << 31) for v in (a, b, tx, ty))
    return a, b, tx, ty, d[0], d[1], len(inl), [valid[i] for i in inl]


def estimate(prev_red, prev_patches, cur_L, g, fit):
    """One frame against its predecessor in similarity mode: (shift [4], warp [8], blocks [nb][6], inliers [nb])."""
    blocks = np.zeros((g.nb, 6), np.int64)
    warp, inliers = np.zeros(8, np.int64), np.zeros(g.nb, np.int64)
    cur_red = mref.reduce_luma(cur_L, g)
    R, k, P = g.R, g.k, g.P
    valid = []
    for b in range(g.nb):
        (dy, dx), smin, smax = mref.best(mref.coarse_sads(prev_red, cur_red, g, b), R)
        blocks[b, :4] = dx, dy, smin, smax
        if mref.block_valid(blocks[b], g):
            valid.append(b)
    n = len(valid)
    if n < g.min_blocks:
        return np.array([0, 0, 0, n], np.int64), warp, blocks, inliers
    for b in valid:                                                  # the window sits at the block's OWN coarse vector
        py, px = g.patch_origin(b)
        cx, cy = int(blocks[b, 0]), int(blocks[b, 1])
        assert abs(cx) <= R and abs(cy) <= R
        tpl, sads = prev_patches[b], {}
        for ey in range(-k, k + 1):
            for ex in range(-k, k + 1):
                y, x = py + cy * k + ey, px + cx * k + ex
                assert 0 <= y and y + P <= g.H and 0 <= x and x + P <= g.W, 'the geometry keeps every read inside the frame'
                sads[(ey, ex)] = int(np.abs(tpl - cur_L[y:y + P, x:x + P]).sum())
        (ey, ex), _, _ = mref.best(sads, k)
        blocks[b, 4:] = cx * k + ex, cy * k + ey
    m = fit_model(g, blocks, valid, fit)
    if m is None:
        return np.array([0, 0, 0, n], np.int64), warp, blocks, inliers
    warp[:] = m[0], m[1], m[2], m[3], m[4], m[5], 1, m[6]
    inliers[m[7]] = 1
    return np.array([(m[2] + 32768) >> 16, (m[3] + 32768) >> 16, 1, n], np.int64), warp, blocks, inliers


class Stream(mref.Stream):
    """mref.Stream in similarity mode."""

    def __init__(self, g, fit):
        super().__init__(g)
        self.fit = fit

    def step(self, L):
        g = self.g
        if self.seen:
            out = estimate(self.reduced, self.patches, L, g, self.fit)
        else:
            out = np.zeros(4, np.int64), np.zeros(8, np.int64), np.zeros((g.nb, 6), np.int64), np.zeros(g.nb, np.int64)
        self.seen, self.reduced, self.patches = 1, mref.reduce_luma(L, g), mref.patches(L, g)
        return out


def run(streams, lumas):
    """lumas int64 [S, F, H, W] through the S streams: dict of shift [S, F, 4], warp [S, F, 8], blocks [S, F, nb, 6], inliers
    [S, F, nb]."""
    S, F = lumas.shape[:2]
    nb = streams[0].g.nb
    out = dict(shift=np.zeros((S, F, 4), np.int64), warp=np.zeros((S, F, 8), np.int64), blocks=np.zeros((S, F, nb, 6), np.int64),
               inliers=np.zeros((S, F, nb), np.int64))
    for s in range(S):
        for f in range(F):
            out['shift'][s, f], out['warp'][s, f], out['blocks'][s, f], out['inliers'][s, f] = streams[s].step(lumas[s, f])
    return out


# ---- the model as a map, and warped test scenes ----

def true_model(deg, zoom, shift):
    """(a, b, tx, ty) as reals of the similarity that turns by deg, zooms by zoom about the frame centre and then shifts."""
    r = math.radians(deg)
    return zoom * math.cos(r) - 1.0, zoom * math.sin(r), float(shift[0]), float(shift[1])


def apply_model(model, hw, x, y):
    """The model p -> p + t + (M - I)(p - c) on real coordinates (model: reals, c the frame centre)."""
    a, b, tx, ty = model
    ux, uy = x - hw[1] / 2.0, y - hw[0] / 2.0
    return x + tx + a * ux - b * uy, y + ty + b * ux + a * uy


def corner_error(warp_row, truth, hw):
    """The largest distance, over the four frame corners, between the estimated model (a warp row, Q16) and the true one."""
    est = tuple(int(v) / ONE for v in warp_row[:4])
    err = 0.0
    for x, y in ((0, 0), (hw[1], 0), (0, hw[0]), (hw[1], hw[0])):
        ex, ey = apply_model(est, hw, x, y)
        gx, gy = apply_model(truth, hw, x, y)
        err = max(err, math.hypot(ex - gx, ey - gy))
    return err


def warped(tex, hw, margin, truth):
    """The frame after `truth` of the frame tex[margin : margin + H, margin : margin + W]: content at p of that crop is at
    model(p) here.  Bilinear samples of the texture at the inverse map, rounded to uint8."""
    H, W = hw
    a, b, tx, ty = truth
    yy, xx = np.mgrid[:H, :W].astype(np.float64)
    vx, vy = xx - tx - W / 2.0, yy - ty - H / 2.0                     # M (p - c) = p' - t - c
    det = (1 + a) ** 2 + b ** 2
    sx = ((1 + a) * vx + b * vy) / det + W / 2.0 + margin
    sy = (-b * vx + (1 + a) * vy) / det + H / 2.0 + margin
    x0, y0 = np.floor(sx).astype(np.int64), np.floor(sy).astype(np.int64)
    assert x0.min() >= 0 and y0.min() >= 0 and x0.max() + 1 < tex.shape[1] and y0.max() + 1 < tex.shape[0], 'the margin is too small'
    fx, fy = sx - x0, sy - y0
    t = tex.astype(np.float64)
    v = (t[y0, x0] * (1 - fx) + t[y0, x0 + 1] * fx) * (1 - fy) + (t[y0 + 1, x0] * (1 - fx) + t[y0 + 1, x0 + 1] * fx) * fy
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


def scene(hw, seed, truths, margin=48, cell=12):
    """Frames uint8 [len(truths) + 1, H, W]: a crop of coarse_texture, then one frame per entry of truths, each the warp of the
    FIRST frame by that entry (so consecutive entries are not composed: the tests use frame pairs or still runs)."""
    tex = mref.coarse_texture(hw[0] + 2 * margin, hw[1] + 2 * margin, seed, cell=cell)
    first = tex[margin:margin + hw[0], margin:margin + hw[1]]
    return np.stack([first] + [warped(tex, hw, margin, t) for t in truths])


# ---- the tracker with the warp ----

def warp_predict(x, v, row, img_hw, box_width):
    """The warp rule of predict on x[5], v[5] after x += v (x[4] not yet reduced), in their own precision: in float32 every line
    is one rounded operation, in the order of the header.  Identity parts are skipped, so that a pure shift row gives the shift
    rule's bits."""
    f32 = x.dtype.type
    a, b, tx, ty, s_q, deg_q = (int(r) for r in row[:6])
    x, v = x.copy(), v.copy()
    scale = f32(1.0 / ONE)
    fa, fb, ftx, fty = f32(a) * scale, f32(b) * scale, f32(tx) * scale, f32(ty) * scale
    ux, uy = x[0] - f32(img_hw[1]) * f32(0.5), x[1] - f32(img_hw[0]) * f32(0.5)
    x[0] = x[0] + ftx
    x[1] = x[1] + fty
    if a != 0 or b != 0:
        x[0] = x[0] + (fa * ux - fb * uy)
        x[1] = x[1] + (fb * ux + fa * uy)
        v0, v1 = v[0], v[1]
        v[0] = v0 + (fa * v0 - fb * v1)
        v[1] = v1 + (fb * v0 + fa * v1)
    if s_q != ONE:
        fs = f32(s_q) * scale
        x[2], x[3], v[2], v[3] = x[2] * fs, x[3] * fs, v[2] * fs, v[3] * fs
    if box_width == 5 and deg_q != 0:
        x[4] = x[4] + f32(deg_q) * scale
    return x, v


class WarpTrack(_track_ref.Track):
    """Track whose predict applies the frame's warp row after x += v: par.warp = (row [8], box_width) or None."""

    def predict(self, par):
        warp = getattr(par, 'warp', None)
        if warp is None:
            return super().predict(par)
        super().predict(par)                                         # x = x + v (kept in box, the angle not reduced); score, missed
        x = self.x.copy()
        x[4] = self.box[4]
        self.x, self.v = warp_predict(x, self.v, warp[0], (par.img_h, par.img_w), warp[1])
        self.box = self.x.copy()
        self.x[4] = _track_ref.mod180(self.x[4])


class WarpStream(_assoc_ref.Stream):
    """_assoc_ref.Stream whose every frame takes a warp row (a, b, tx, ty, s_q, deg_q, valid, n_inliers), or None."""

    def __init__(self, max_tracks, par, box_width, **kw):
        super().__init__(max_tracks, par, **kw)
        self.box_width = box_width

    def step(self, boxes, scores, cats, count, warp=None):
        self.par.warp = None if warp is None or int(warp[6]) != 1 else (np.asarray(warp), self.box_width)
        for t in self.slots:
            if t is not None:
                t.__class__ = WarpTrack
        out = super().step(boxes, scores, cats, count)
        self.par.warp = None
        return out


def run_tracker(frames, warps, width, img_hw, max_tracks=16, params=None, assoc=None, dtype=np.float32):
    """Wire-record frames through a fresh WarpStream: (stream, the outputs of every frame, the state arrays after every
    frame)."""
    par = _track_ref.Params(img_hw, dtype, **dict(dict(match='iou'), **(params or {})))
    stream = WarpStream(max_tracks, par, width, **(assoc or {}))
    outs, arrays = [], []
    for f, r in enumerate(_track_ref.pack_records(frames, width)):
        outs.append(stream.step(*_track_ref.unpack_frame(r, width), warp=None if warps is None else warps[f]))
        arrays.append(stream.arrays())
    return stream, outs, arrays
