"""The camera-motion rules of include/mydet.h (mydet_motion_frames_rgb_u8) in Python integers and numpy, and the tracker with
the shift (mydet_track_frames_motion_f32) on top of tests/_track_ref.py and tests/_assoc_ref.py (test code; the package never
imports it).  Written from the rule text, not from the kernels: whole-image differences and sorts where the kernels use LDS
windows, packed keys and histograms."""
import numpy as np

import _assoc_ref
import _track_ref


# ---- luma ----

def luma_rgb(frames):
    """uint8 [..., H, W, 3] -> int64 [..., H, W]."""
    f = np.asarray(frames).astype(np.int64)
    return (77 * f[..., 0] + 150 * f[..., 1] + 29 * f[..., 2] + 128) >> 8


def luma_y(y, layout):
    """A Y plane as the layout stores it (uint8, or 16-bit words for 'p010' / 'i010') -> int64, 0 .. 255."""
    y = np.asarray(y)
    if layout in ('p010', 'i010'):
        w = y.view(np.uint16).astype(np.int64)
        v10 = (w >> 6) if layout == 'p010' else (w & 1023)
        return np.minimum(255, (v10 + 2) >> 2)
    return y.astype(np.int64)


# ---- geometry ----

class Geometry:
    def __init__(self, frame_hw, reduce=None, search=8, min_texture=1024, min_blocks=None):
        H, W = (int(v) for v in frame_hw)
        if reduce is None:
            reduce = next((k for k in (2, 4) if max(H, W) <= 512 * k), 8)
        assert reduce in (2, 4, 8) and 4 <= search <= 16
        self.H, self.W, self.k, self.R = H, W, reduce, search
        self.hr, self.wr = H // reduce, W // reduce
        assert min(self.hr, self.wr) >= 2 * search + 16, 'MYDET_E_BADARG'
        self.nby, self.nbx = (self.hr - 2 * search) // 16, (self.wr - 2 * search) // 16
        self.nb = self.nby * self.nbx
        assert self.nb <= 1024, 'MYDET_E_UNSUPP'
        self.P = min(32, 8 * reduce)
        self.min_texture = int(min_texture)
        self.min_blocks = max(2, -(-self.nb // 8)) if min_blocks is None else int(min_blocks)

    def origin(self, b):
        """(y0, x0) of block b in the previous reduced luma."""
        return self.R + 16 * (b // self.nbx), self.R + 16 * (b % self.nbx)

    def patch_origin(self, b):
        y0, x0 = self.origin(b)
        return (y0 + 8) * self.k - self.P // 2, (x0 + 8) * self.k - self.P // 2


def reduce_luma(L, g):
    k = g.k
    box = L[:g.hr * k, :g.wr * k].reshape(g.hr, k, g.wr, k).sum(axis=(1, 3))
    return (box + k * k // 2) >> (k * k).bit_length() - 1


def patches(L, g):
    out = np.zeros((g.nb, g.P, g.P), np.int64)
    for b in range(g.nb):
        py, px = g.patch_origin(b)
        out[b] = L[py:py + g.P, px:px + g.P]
    return out


def lower_median(values):
    v = sorted(int(x) for x in values)
    return v[(len(v) - 1) // 2]


def best(sads, r):
    """sads[(dy, dx)] -> ((dy, dx) of the smallest (SAD, dy^2 + dx^2, dy, dx), its SAD, the largest SAD)."""
    key = min((s, dy * dy + dx * dx, dy, dx) for (dy, dx), s in sads.items())
    return (key[2], key[3]), key[0], max(sads.values())


def coarse_sads(prev_red, cur_red, g, b):
    """sads[(dy, dx)] of block b of the previous reduced luma against the current one, every (dy, dx) in [-R, R]^2."""
    y0, x0 = g.origin(b)
    tpl = prev_red[y0:y0 + 16, x0:x0 + 16]
    return {(dy, dx): int(np.abs(tpl - cur_red[y0 + dy:y0 + dy + 16, x0 + dx:x0 + dx + 16]).sum())
            for dy in range(-g.R, g.R + 1) for dx in range(-g.R, g.R + 1)}


def block_valid(row, g):
    """Whether a block row (cdx, cdy, smin, smax, ...) is VALID under g.min_texture."""
    smin, smax = int(row[2]), int(row[3])
    return smax - smin >= g.min_texture and 2 * smin <= smax


def estimate(prev_red, prev_patches, cur_L, g):
    """One frame against its predecessor: (shift [4], blocks [nb][6])."""
    blocks = np.zeros((g.nb, 6), np.int64)
    cur_red = reduce_luma(cur_L, g)
    R, k, P = g.R, g.k, g.P
    valid = []
    for b in range(g.nb):
        (dy, dx), smin, smax = best(coarse_sads(prev_red, cur_red, g, b), R)
        blocks[b, :4] = dx, dy, smin, smax
        if block_valid(blocks[b], g):
            valid.append(b)
    n = len(valid)
    if n < g.min_blocks:
        return np.array([0, 0, 0, n], np.int64), blocks
    Dx, Dy = lower_median(blocks[valid, 0]), lower_median(blocks[valid, 1])
    for b in valid:
        py, px = g.patch_origin(b)
        tpl = prev_patches[b]
        sads = {}
        for ey in range(-k, k + 1):
            for ex in range(-k, k + 1):
                y, x = py + Dy * k + ey, px + Dx * k + ex
                assert 0 <= y and y + P <= g.H and 0 <= x and x + P <= g.W, 'the geometry keeps every read inside the frame'
                sads[(ey, ex)] = int(np.abs(tpl - cur_L[y:y + P, x:x + P]).sum())
        (ey, ex), _, _ = best(sads, k)
        blocks[b, 4:] = Dx * k + ex, Dy * k + ey
    return np.array([lower_median(blocks[valid, 4]), lower_median(blocks[valid, 5]), 1, n], np.int64), blocks


class Stream:
    """The estimator state of one stream: seen, and the reduced luma and the patches of the last frame."""

    def __init__(self, g):
        self.g, self.seen = g, 0
        self.reduced = np.zeros((g.hr, g.wr), np.int64)
        self.patches = np.zeros((g.nb, g.P, g.P), np.int64)

    def step(self, L):
        g = self.g
        if self.seen:
            shift, blocks = estimate(self.reduced, self.patches, L, g)
        else:
            shift, blocks = np.zeros(4, np.int64), np.zeros((g.nb, 6), np.int64)
        self.seen, self.reduced, self.patches = 1, reduce_luma(L, g), patches(L, g)
        return shift, blocks


def run(streams, lumas):
    """lumas int64 [S, F, H, W] through the S streams: (shift [S, F, 4], blocks [S, F, nb, 6])."""
    S, F = lumas.shape[:2]
    g = streams[0].g
    shift, blocks = np.zeros((S, F, 4), np.int64), np.zeros((S, F, g.nb, 6), np.int64)
    for s in range(S):
        for f in range(F):
            shift[s, f], blocks[s, f] = streams[s].step(lumas[s, f])
    return shift, blocks


# ---- test textures ----

def _box_mean(raw, h, w, smooth):
    acc = np.zeros((h, w), np.int64)
    for i in range(smooth):
        for j in range(smooth):
            acc += raw[i:i + h, j:j + w]
    return ((acc + smooth * smooth // 2) // (smooth * smooth)).astype(np.uint8)


def texture(h, w, seed, smooth=5):
    """Uniform noise smoothed by a smooth x smooth box mean, uint8 [h, w] (raw noise aliases in the reduced images)."""
    rng = np.random.default_rng(seed)
    return _box_mean(rng.integers(0, 256, (h + smooth - 1, w + smooth - 1)).astype(np.int64), h, w, smooth)


def coarse_texture(h, w, seed, cell=12, smooth=5, saturate=0):
    """Uniform noise replicated in cell x cell cells, then the box mean: texture() is too fine for k = 8 (a block's SAD range
    stays below the default min_texture), this is not.  saturate: cell values are drawn from 0 .. 255 + saturate and clipped,
    so that about saturate / 256 of the cells are 255, and stay 255 inside the cell (cell > smooth)."""
    rng = np.random.default_rng(seed)
    hh, ww = h + smooth - 1, w + smooth - 1
    cells = np.minimum(255, rng.integers(0, 256 + saturate, (-(-hh // cell), -(-ww // cell))))
    return _box_mean(cells.repeat(cell, axis=0).repeat(cell, axis=1)[:hh, :ww].astype(np.int64), h, w, smooth)


def crops(tex, hw, offsets):
    """Crops of one texture: frame i shows tex[oy : oy + H, ox : ox + W]; content at p in frame i-1 is at p + d in frame i with
    d = (ox[i-1] - ox[i], oy[i-1] - oy[i])."""
    H, W = hw
    return np.stack([tex[oy:oy + H, ox:ox + W] for oy, ox in offsets])


def offsets_of_shifts(shifts, margin):
    """Crop origins (oy, ox) of len(shifts) + 1 frames whose consecutive true shifts are `shifts` [(dx, dy)], from (margin, margin)."""
    oy, ox, out = margin, margin, [(margin, margin)]
    for dx, dy in shifts:
        oy, ox = oy - dy, ox - dx
        out.append((oy, ox))
    return out


# ---- test scenes whose blocks disagree ----

def two_motions(tex_a, tex_b, hw, shifts_a, shifts_b, mask, margin):
    """Frames uint8 [len(shifts) + 1, H, W] of two regions: where `mask` (bool [H, W]) is False crops of tex_a that move by
    shifts_a, where it is True crops of tex_b that move by shifts_b.  The regions stay where they are; their content moves."""
    a = crops(tex_a, hw, offsets_of_shifts(shifts_a, margin))
    b = crops(tex_b, hw, offsets_of_shifts(shifts_b, margin))
    return np.where(mask[None], b, a)


def partly_flat(frames, mask, value=90):
    """The frames with the region `mask` (bool [H, W]) at one constant luma: blocks that see nothing else are invalid."""
    out = frames.copy()
    out[..., mask] = value
    return out


def periodic(hw, period_yx, shift, seed, margin=32):
    """Two frames uint8 [2, H, W] of a texture that repeats every period_yx[0] rows and period_yx[1] columns (None: does not
    repeat along that axis), the second moved by shift = (dx, dy): candidates a whole period apart have equal SADs."""
    H, W = hw
    py, px = period_yx
    tile = texture(py or H + 2 * margin, px or W + 2 * margin, seed)
    big = np.tile(tile, (-(-(H + 2 * margin) // tile.shape[0]), -(-(W + 2 * margin) // tile.shape[1])))
    return crops(big, hw, offsets_of_shifts([shift], margin))


def diagonal(hw, period, shift, seed, margin=32):
    """Two frames uint8 [2, H, W] of a texture that repeats only under the translation (dx, dy) = (period / 2, -period / 2) and
    its multiples, the second moved by shift = (dx, dy): with shift = (period / 4, -period / 4) the candidates (dx, dy) and
    (-dx, -dy) tie at the same distance, and the order of dy and dx in the comparison decides."""
    H, W = hw
    yy, xx = np.mgrid[:H + 2 * margin, :W + 2 * margin]
    along = texture(H + W + 4 * margin, period, seed)
    return crops(along[xx + yy, (xx - yy) % period], hw, offsets_of_shifts([shift], margin))


def store_y(y8, layout, rng):
    """The 8-bit luma y8 as the Y plane of `layout` stores it: uint8, or int16 words of ten live bits v10 = clip(4 y + j, 0,
    1023) with a random j in [-2, 1] (up to +3 where y = 255: the clamp of the 10-bit rule) and six random ignored bits."""
    if layout not in ('p010', 'i010'):
        return y8.astype(np.uint8)
    y = y8.astype(np.int64)
    j = rng.integers(-2, 2, y.shape)
    j = np.where(y == 255, rng.integers(-2, 4, y.shape), j)
    v10 = np.clip(4 * y + j, 0, 1023).astype(np.uint16)
    junk = rng.integers(0, 64, y.shape).astype(np.uint16)
    return ((v10 << 6) | junk if layout == 'p010' else v10 | (junk << 10)).view(np.int16)


def live_bits(stored, layout):
    """The ten live bits of 16-bit words as the layout stores them, int64."""
    w = np.asarray(stored).view(np.uint16).astype(np.int64)
    return (w >> 6) if layout == 'p010' else (w & 1023)


def medians(values):
    """(lower, upper) median of a list of integers."""
    v = sorted(int(x) for x in values)
    return v[(len(v) - 1) // 2], v[len(v) // 2]


# ---- the tracker with the shift ----

class ShiftTrack(_track_ref.Track):
    """Track whose predict adds the frame's shift after x += v (mydet_track_frames_motion_f32): par.shift = (dx, dy) or None."""

    def predict(self, par):
        shift = getattr(par, 'shift', None)
        if shift is None:
            return super().predict(par)
        v = self.v.copy()
        super().predict(par)                                         # x = x + v; the angle reduced; score and missed
        dt = par.dtype
        self.x[0] = self.x[0] + dt(shift[0])
        self.x[1] = self.x[1] + dt(shift[1])
        self.box[:2] = self.x[:2]
        assert np.array_equal(self.v, v)                             # velocities are untouched


class ShiftStream(_assoc_ref.Stream):
    """_assoc_ref.Stream whose every frame takes a row of the estimator's output (dx, dy, valid, n_valid), or None."""

    def step(self, boxes, scores, cats, count, shift=None):
        self.par.shift = None if shift is None or int(shift[2]) != 1 else (int(shift[0]), int(shift[1]))
        for t in self.slots:
            if t is not None:
                t.__class__ = ShiftTrack
        out = super().step(boxes, scores, cats, count)
        self.par.shift = None
        return out


TRACK_HW = (480, 640)
TRACK_SHIFTS = ((20, -12), (-18, 14))


def tracker_scenario(frames=8, width=4, still=None, low_from=None):
    """Three boxes of about 24 px that drift slowly while the camera jerks: frame f > 0 moves the whole image by
    TRACK_SHIFTS[(f - 1) % 2], except frame `still`, where the camera rests and the estimator reports valid = 0.  Returns
    (frames for _track_ref.pack_records, shift rows int32 [frames, 4]).  low_from: from that frame on the third box scores 0.45
    (a LOW detection for a tracker with bands)."""
    base = np.array([[200.0, 150.0, 24.0, 26.0, 10.0], [330.0, 250.0, 22.0, 24.0, 0.0], [440.0, 330.0, 26.0, 24.0, 170.0]])
    drift = np.array([[1.0, 0.5], [-0.5, 1.0], [0.75, -0.75]])
    cats = np.array([0, 0, 1], np.int64)
    cam, out, shifts = np.zeros(2), [], np.zeros((frames, 4), np.int32)
    for f in range(frames):
        if f > 0 and f != still:
            d = TRACK_SHIFTS[(f - 1) % 2]
            cam = cam + d
            shifts[f] = d[0], d[1], 1, 6
        b = base.copy()
        b[:, :2] += drift * f + cam
        scores = np.array([0.9, 0.8, 0.45 if low_from is not None and f >= low_from else 0.7], np.float32)
        out.append((b[:, :width].astype(np.float32), scores, cats))
    return out, shifts


def run_tracker(frames, shifts, width, dtype, max_tracks=16, params=None, assoc=None):
    """The scenario through a fresh ShiftStream: (stream, the outputs of every frame, the state arrays after every frame)."""
    par = _track_ref.Params(TRACK_HW, dtype, match='iou', **(params or {}))
    stream = ShiftStream(max_tracks, par, **(assoc or {}))
    outs, arrays = [], []
    for f, r in enumerate(_track_ref.pack_records(frames, width)):
        outs.append(stream.step(*_track_ref.unpack_frame(r, width), shift=None if shifts is None else shifts[f]))
        arrays.append(stream.arrays())
    return stream, outs, arrays
