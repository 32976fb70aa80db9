"""Case generator shared by tests/test_crop_host.py and tests/test_gpu_crop.py.  Every box has cx, cy, w, h at multiples of 1/8
and a size that is the chip size times 0.75, 1.5 or 5 (times pad 1.0 or 1.25), so in axis-aligned boxes and quarter turns
every sample point is exact in float32 and lands on an odd multiple of 1/64 pixel: settled (tests/_crop_ref.py).  Only the
angle of the rotated cases is inexact.  Reference chips are computed once per case and shared (ref_chips)."""
import functools

import numpy as np

import _crop_ref as ref

SIZES = ((96, 160), (95, 157))           # B = 2 frames of each; the second odd in both directions
CHIPS = ((16, 8), (32, 16), (13, 7))     # (height, width): two take the wide stores, the last one the element path
PADS = (1.0, 1.25)
SCALES = (0.75, 1.5, 5.0)                # below 1 (one sample), 2 x 2 samples, the clamp to 4 x 4
FILL = (7, 201, 94)
KINDS = ('contiguous', 'pitched', 'odd')


def frames(H, W, seed=0):
    """uint8 [2, H, W, 3]: a smooth picture plus noise, every value 0..255 present."""
    rng = np.random.default_rng(1000 + seed + H)
    y, x = np.mgrid[0:H, 0:W]
    base = np.stack([128 + 100 * np.sin(x / 9.0 + b) * np.cos(y / 7.0 + c) for b in range(2) for c in range(3)]).reshape(2, 3, H, W)
    img = np.moveaxis(base, 1, -1) + rng.integers(-28, 29, size=(2, H, W, 3))
    img = np.clip(img, 0, 255).astype(np.uint8)
    img[:, 0, :, 0] = (np.arange(W) * 255 // (W - 1)).astype(np.uint8)
    return img


def axis_rows(H, W, chip):
    """float32 [K, 5]: axis-aligned boxes at every scale, inside, over each edge and wholly outside the frame; the same at the
    quarter turns; and the rows that are no boxes (they get a fill chip)."""
    ch, cw = chip
    a, b, c = SCALES
    nan, inf = float('nan'), float('inf')
    rows = [[40.5, 30.25, cw * a, ch * a, 0], [80.125, 48.0, cw * b, ch * b, 0], [W / 2, H / 2, cw * c, ch * c, 0],
            [0.0, 20.0, cw * b, ch * a, 0], [W + 0.0, H + 0.0, cw * b, ch * b, 0], [60.375, -2.0, cw * a, ch * b, 0],
            [70.0, 40.0, cw * c, ch * a, 0], [W - 3.5, 50.125, cw * a, ch * c, 0],
            [-100.0, -100.0, cw * b, ch * b, 0], [3e9, 10.0, cw * b, ch * b, 0],                  # wholly outside
            [40.5, 30.25, cw * a, ch * a, 90], [80.125, 48.0, cw * b, ch * b, 180], [70.0, 40.0, cw * c, ch * a, 270],
            [0.0, 20.0, cw * b, ch * a, -90], [W + 0.0, H + 0.0, cw * b, ch * b, 450], [60.375, -2.0, cw * a, ch * b, -180],
            [nan, 50.0, 10.0, 10.0, 0], [50.0, 50.0, inf, 10.0, 0], [50.0, 50.0, 0.0, 10.0, 0], [50.0, 40.0, 10.0, -4.0, 0],
            [50.0, 50.0, 10.0, 10.0, nan]]
    return np.asarray(rows, dtype=np.float32)


SKIPPED_ROWS = 5                         # the last rows of axis_rows


def rotated_rows(H, W, chip):
    """float32 [K, 5]: boxes at 30, -45 and 200 degrees, one and 2 x 2 samples per pixel, inside and over the frame's edges."""
    ch, cw = chip
    a, b, _ = SCALES
    rows = [[40.5, 30.25, cw * a, ch * a, 30], [80.125, 48.0, cw * b, ch * b, 30], [3.0, 20.0, cw * b, ch * a, 30],
            [60.5, 40.0, cw * a, ch * b, -45], [100.25, 60.0, cw * b, ch * b, -45], [W - 2.0, H - 4.0, cw * b, ch * b, -45],
            [50.0, 50.5, cw * b, ch * a, 200], [120.125, 30.0, cw * a, ch * a, 200], [70.0, 2.0, cw * b, ch * b, 200]]
    return np.asarray(rows, dtype=np.float32)


def case_boxes(kind, H, W, chip):
    """(boxes float32 [2, K, 5], counts int32 [2]): frame 0 every row, frame 1 the rows in reverse order, all but its last two."""
    rows = axis_rows(H, W, chip) if kind == 'axis' else rotated_rows(H, W, chip)
    return np.stack([rows, rows[::-1]]).copy(), np.array([len(rows), len(rows) - 2], dtype=np.int32)


def all_cases():
    """(kind, size index, chip, pad) of every case."""
    return [(kind, n, chip, pad) for kind in ('axis', 'rotated') for n in range(len(SIZES)) for chip in CHIPS for pad in PADS]


@functools.lru_cache(maxsize=None)
def ref_chips(kind, n, chip, pad):
    """The restatement's (value, lo, hi, written) for a case on frames(*SIZES[n]); computed once, never modified."""
    H, W = SIZES[n]
    boxes, counts = case_boxes(kind, H, W, chip)
    out = ref.chips(frames(H, W), boxes, chip, pad, FILL, counts)
    for a in out:
        a.setflags(write=False)
    return out


class Target:
    """B planes / frames [B, H, W(, C)] of random bytes (or of `data`) inside a random backing buffer on the device, plus the
    host copy -- the three target kinds of tests/test_gpu_draw.py: contiguous; a pitch and frame stride that are multiples
    of 4 but not the row's bytes; a crop view at odd byte offsets inside a larger buffer."""

    def __init__(self, rng, B, H, W, C, kind, data=None, avoid=None):
        import torch
        if kind == 'contiguous':
            pad_y, pad_x, oy, ox, lead = 0, 0, 0, 0, 0
        elif kind == 'pitched':                                       # base, pitch and frame stride multiples of 4; W is not the pitch
            pad_x = 4 + (-(W + 4) * max(C, 1)) % 4
            while ((W + pad_x) * max(C, 1)) % 4:
                pad_x += 1
            pad_y, oy, ox, lead = 0, 0, 0, 0
        else:
            pad_y, pad_x, oy, ox, lead = 5, 7, 2, 3, 1
            if ((W + pad_x) * max(C, 1)) % 2 == 0:
                pad_x += 1                                           # an odd pitch as well
        shape = (B, H + pad_y, W + pad_x) + ((C,) if C else ())
        self.back = rng.integers(0, 256, size=shape, dtype=np.uint8)
        if avoid is not None:                                        # no pixel of the backing buffer has this colour
            hit = (self.back == np.asarray(avoid, dtype=np.uint8)).all(axis=-1)
            self.back[hit, 0] ^= 0x80
        if data is not None:
            self.back[:, oy:oy + H, ox:ox + W] = data
        self.lead = rng.integers(0, 256, size=lead, dtype=np.uint8)
        self.flat = torch.from_numpy(np.concatenate([self.lead, self.back.ravel()])).cuda()
        self.view = self.flat[lead:].view(shape)[:, oy:oy + H, ox:ox + W]
        self.host = self.back[:, oy:oy + H, ox:ox + W]
        self.n_lead, self.oy, self.ox = lead, oy, ox
