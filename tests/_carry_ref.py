"""The rules of the key-frame carry (include/mydet.h: mydet_carry_records_rgb_u8) restated in Python integers: the checker of
tests/test_gpu_carry.py, held to known motions by tests/test_carry_host.py.  One float32 conversion of the box, one float32 add
per emitted centre; everything else is integer arithmetic, so the kernels equal this with ==."""
import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

SLOTS, SLOT_WORDS, HEADER = 512, 336, 16
REC_COUNT, REC_BBOX = 0, 4
REC_SCORE = REC_BBOX + 4 * SLOTS
REC_CLASS = REC_SCORE + SLOTS
REC_INDEX = REC_CLASS + 2 * SLOTS
REC_WORDS = REC_INDEX + SLOTS
REC_ANGLE = REC_WORDS
REC_ROT_WORDS = REC_WORDS + SLOTS
NONE, KEY, CARRIED, FLAT, LOST, LEFT, NOT = range(7)
C_LIMIT = 65536


def luma_rgb(frames):
    """int64 [..., H, W] of uint8 [..., H, W, 3]."""
    f = frames.astype(np.int64)
    return (77 * f[..., 0] + 150 * f[..., 1] + 29 * f[..., 2] + 128) >> 8


def luma_y(y, layout):
    """int64 luma of a Y plane: the sample itself, or the 10-bit rule of 'p010' (high bits) and 'i010' (low bits)."""
    if layout in ('p010', 'i010'):
        w = y.astype(np.int64) & 0xffff
        v10 = (w >> 6) if layout == 'p010' else (w & 1023)
        return np.minimum(255, (v10 + 2) >> 2)
    return y.astype(np.int64)


def record(boxes, scores=None, classes=None, angles=None, count=None):
    """An int32 record row of float boxes [n, 4] (rotated with `angles`)."""
    n = len(boxes)
    r = np.zeros(REC_WORDS if angles is None else REC_ROT_WORDS, np.int32)
    r[REC_COUNT] = n if count is None else count
    r[REC_BBOX:REC_BBOX + 4 * n] = np.asarray(boxes, np.float32).reshape(-1).view(np.int32)
    r[REC_SCORE:REC_SCORE + n] = (np.linspace(0.9, 0.5, n) if scores is None else np.asarray(scores)).astype(np.float32).view(np.int32)
    r[REC_CLASS:REC_CLASS + 2 * n] = (np.arange(n) % 5 if classes is None else np.asarray(classes)).astype(np.int64).view(np.int32)
    r[REC_INDEX:REC_INDEX + n] = np.arange(n) * 7
    if angles is not None:
        r[REC_ANGLE:REC_ANGLE + n] = np.asarray(angles, np.float32).view(np.int32)
    return r


def to_fixed(v):
    """(ok, v16) of a float32: floor(v * 16 + 0.5) with a separate float32 multiply and add."""
    v = np.float32(v)
    if not np.abs(v) < np.float32(67108864.0):
        return False, 0
    return True, int(np.floor(np.float32(np.float32(v * np.float32(16.0)) + np.float32(0.5))))


def gather(L, y0, x0, h, w):
    """L at rows y0 .. y0 + h - 1 and columns x0 .. x0 + w - 1, coordinates clamped to the frame."""
    ys = np.clip(np.arange(y0, y0 + h), 0, L.shape[0] - 1)
    xs = np.clip(np.arange(x0, x0 + w), 0, L.shape[1] - 1)
    return L[ys][:, xs]


def means(L, y0, x0, s, n):
    """n x n means of s x s cells from (y0, x0)."""
    g = gather(L, y0, x0, n * s, n * s).reshape(n, s, n, s).sum(axis=(1, 3))
    return (g + s * s // 2) // (s * s)


def search(tpl, win, r):
    """The best (SAD, dy*dy + dx*dx, dy, dx) of template `tpl` [n, n] in window `win` [n + 2r, n + 2r]: (dy, dx, smin, smax)."""
    n = tpl.shape[0]
    sad = np.abs(sliding_window_view(win, (n, n)) - tpl).sum(axis=(2, 3))
    d = np.arange(-r, r + 1)
    dy, dx = np.meshgrid(d, d, indexing='ij')
    order = np.lexsort((dx.ravel(), dy.ravel(), (dy * dy + dx * dx).ravel(), sad.ravel()))
    b = order[0]
    return int(dy.ravel()[b]), int(dx.ravel()[b]), int(sad.ravel()[b]), int(sad.max())


class Slot:
    def __init__(self):
        self.status = NONE
        self.clear()

    def clear(self):
        self.s = self.cx16 = self.cy16 = 0
        self.off, self.rel = [0, 0], [0, 0]
        self.key = np.zeros(8, np.int32)
        self.coarse, self.patch = np.zeros((16, 16), np.int64), np.zeros((32, 32), np.int64)

    def words(self):
        w = np.zeros(SLOT_WORDS, np.int32)
        w[0] = self.status
        if self.status == CARRIED:
            w[1:8] = [self.s, self.cx16, self.cy16, self.off[0], self.off[1], self.rel[0], self.rel[1]]
            w[8:16] = self.key
            w[HEADER:HEADER + 64] = self.coarse.astype(np.uint8).reshape(-1).view(np.int32)
            w[HEADER + 64:] = self.patch.astype(np.uint8).reshape(-1).view(np.int32)
        return w


class Stream:
    def __init__(self):
        self.slots = [Slot() for _ in range(SLOTS)]
        self.key = None                                              # the record the alive slots came from

    def words(self):
        return np.concatenate([sl.words() for sl in self.slots])


class Settings:
    def __init__(self, every=4, search=8, min_texture=1024, max_diff=24):
        self.every, self.search, self.min_texture, self.max_diff = every, search, min_texture, max_diff


def key_mask(first, every, F):
    return [(first + f) % every == 0 for f in range(F)]


def take_key(stream, L, rec, rot):
    cnt = int(rec[REC_COUNT])
    stream.key = rec
    how = np.zeros(SLOTS, np.int64)
    for j, sl in enumerate(stream.slots):
        sl.status = NONE
        sl.clear()
        if not (1 <= cnt <= SLOTS and j < cnt):
            continue
        how[j] = KEY
        box = rec[REC_BBOX + 4 * j:REC_BBOX + 4 * j + 4].view(np.float32)
        fixed = [to_fixed(v) for v in box]
        if not all(ok for ok, _ in fixed) or fixed[2][1] <= 0 or fixed[3][1] <= 0:
            sl.status = NOT
            continue
        sl.status = CARRIED
        sl.cx16, sl.cy16 = fixed[0][1], fixed[1][1]
        m = min(fixed[2][1], fixed[3][1])
        side = m // 2 if rot else 3 * m // 4
        sl.s = s = min(max((side + 255) // 256, 1), 16)
        sl.key[:4] = rec[REC_BBOX + 4 * j:REC_BBOX + 4 * j + 4]
        sl.key[4] = rec[REC_ANGLE + j] if rot else 0
        sl.key[5] = rec[REC_SCORE + j]
        sl.key[6:8] = rec[REC_CLASS + 2 * j:REC_CLASS + 2 * j + 2]
        X, Y = sl.cx16 >> 4, sl.cy16 >> 4
        sl.coarse = means(L, Y - 8 * s, X - 8 * s, s, 16)
        sl.patch = gather(L, Y - 16, X - 16, 32, 32) if s >= 2 else np.zeros((32, 32), np.int64)
    return how


def follow(sl, L, cfg, shift):
    """Rule 2 for an alive slot in luma L; returns (smin, smax)."""
    H, W = L.shape
    dx, dy = (int(np.clip(shift[0], -C_LIMIT, C_LIMIT)), int(np.clip(shift[1], -C_LIMIT, C_LIMIT))) if shift is not None and shift[2] == 1 else (0, 0)
    cx = int(np.clip(sl.off[0] + sl.rel[0] + dx, -C_LIMIT, C_LIMIT))
    cy = int(np.clip(sl.off[1] + sl.rel[1] + dy, -C_LIMIT, C_LIMIT))
    s, R = sl.s, cfg.search
    X, Y = sl.cx16 >> 4, sl.cy16 >> 4
    win = means(L, Y - 8 * s + cy - R * s, X - 8 * s + cx - R * s, s, 16 + 2 * R)
    i, j, smin, smax = search(sl.coarse, win, R)
    if smax - smin < cfg.min_texture:
        sl.status = FLAT
    elif smin > 256 * cfg.max_diff:
        sl.status = LOST
    else:
        nx, ny = cx + j * s, cy + i * s
        if s >= 2:
            ey, ex, _, _ = search(sl.patch, gather(L, Y - 16 + ny - s, X - 16 + nx - s, 32 + 2 * s, 32 + 2 * s), s)
            nx, ny = nx + ex, ny + ey
        sl.rel = [nx - sl.off[0] - dx, ny - sl.off[1] - dy]
        sl.off = [nx, ny]
        if not (0 <= X + nx < W and 0 <= Y + ny < H):
            sl.status = LEFT
    if sl.status != CARRIED:
        sl.clear()
    return smin, smax


def emit(stream, rot):
    out = np.zeros(REC_ROT_WORDS if rot else REC_WORDS, np.int32)
    d = 0
    for j, sl in enumerate(stream.slots):
        if sl.status != CARRIED:
            continue
        box = sl.key[:4].view(np.float32).copy()
        box[0] = np.float32(box[0] + np.float32(sl.off[0]))
        box[1] = np.float32(box[1] + np.float32(sl.off[1]))
        out[REC_BBOX + 4 * d:REC_BBOX + 4 * d + 4] = box.view(np.int32)
        out[REC_SCORE + d] = sl.key[5]
        out[REC_CLASS + 2 * d:REC_CLASS + 2 * d + 2] = sl.key[6:8]
        out[REC_INDEX + d] = j
        if rot:
            out[REC_ANGLE + d] = sl.key[4]
        d += 1
    out[REC_COUNT] = d
    return out


def run(streams, lumas, key_records, first, cfg, rot=False, shift=None):
    """The rules on S streams x F frames.  lumas: int64 [S, F, H, W]; key_records: per stream the int32 rows of its key frames, in
    order; first: the place of frame 0 inside its interval; shift: None or int [S, F, 4].  Updates `streams`; returns (records
    int32 [S, F, words], how [S, F, 512], offset [S, F, 512, 2], sad [S, F, 512, 2])."""
    S, F = len(streams), lumas.shape[1]
    words = REC_ROT_WORDS if rot else REC_WORDS
    rec = np.zeros((S, F, words), np.int32)
    how, off, sad = np.zeros((S, F, SLOTS), np.int64), np.zeros((S, F, SLOTS, 2), np.int64), np.zeros((S, F, SLOTS, 2), np.int64)
    for s, st in enumerate(streams):
        k = 0
        for f, is_key in enumerate(key_mask(first, cfg.every, F)):
            if is_key:
                how[s, f] = take_key(st, lumas[s, f], key_records[s][k], rot)
                rec[s, f] = key_records[s][k]
                k += 1
                continue
            for j, sl in enumerate(st.slots):
                if sl.status == CARRIED:
                    sad[s, f, j] = follow(sl, lumas[s, f], cfg, None if shift is None else shift[s, f])
                    if sl.status == CARRIED:
                        off[s, f, j] = sl.off
                how[s, f, j] = sl.status
            rec[s, f] = emit(st, rot)
    return rec, how, off, sad
