"""The inputs of the key-frame carry tests: small synthetic videos whose truth is known.  A textured background, textured
rectangles that move by whole pixels per frame, a flat region; the key records hold the true boxes.  Frames are about 96 x 128,
2 streams x 6 frames with a key frame every 3."""
import functools

import numpy as np

import _carry_ref as ref

HW = (96, 128)
F, EVERY = 6, 3
SETTINGS = dict(every=EVERY, search=4, min_texture=1024, max_diff=24)


def texture(h, w, seed, block=4):
    """uint8 [h, w, 3]: random blocks of `block` pixels under fine noise -- unique under whole-pixel motion, smooth enough at an edge."""
    rng = np.random.Generator(np.random.PCG64(seed))
    coarse = rng.integers(0, 216, size=((h + block - 1) // block, (w + block - 1) // block, 3))
    fine = rng.integers(0, 40, size=(h, w, 3))
    return (np.repeat(np.repeat(coarse, block, axis=0), block, axis=1)[:h, :w] + fine).astype(np.uint8)


class Thing:
    """A textured rectangle of size (h, w) whose centre is at `start` = (cx, cy) in frame 0 and moves along `path`: one (dx, dy) step
    per frame, or a list of steps.  repaint: the frames in which it shows another texture."""

    def __init__(self, name, size, start, path, seed, repaint=()):
        self.name, self.size, self.start, self.seed, self.repaint = name, size, start, seed, tuple(repaint)
        self.path = path

    def centre(self, f):
        steps = [self.path] * f if isinstance(self.path, tuple) else list(self.path[:f])
        return self.start[0] + sum(s[0] for s in steps), self.start[1] + sum(s[1] for s in steps)

    def box(self, f):
        cx, cy = self.centre(f)
        return [cx, cy, self.size[1], self.size[0]]

    def paste(self, frame, f):
        h, w = self.size
        cx, cy = self.centre(f)
        x0, y0 = cx - w // 2, cy - h // 2
        tex = texture(h, w, self.seed + (1000 if f in self.repaint else 0))
        ya, yb, xa, xb = max(y0, 0), min(y0 + h, frame.shape[0]), max(x0, 0), min(x0 + w, frame.shape[1])
        if ya < yb and xa < xb:
            frame[ya:yb, xa:xb] = tex[ya - y0:yb - y0, xa - x0:xb - x0]


class Scene:
    """hw, a background seed, flat regions (y0, x0, h, w) of one colour, things; camera: per frame the (dx, dy) the whole content
    has moved by since frame 0 (None: a fixed camera)."""

    def __init__(self, hw, seed, things, flat=(), camera=None):
        self.hw, self.seed, self.things, self.flat, self.camera = hw, seed, things, flat, camera

    def frame(self, f):
        H, W = self.hw
        m = 64
        bg = texture(H + 2 * m, W + 2 * m, self.seed)
        for y0, x0, h, w in self.flat:
            bg[m + y0:m + y0 + h, m + x0:m + x0 + w] = (90, 140, 60)
        big = bg
        for t in self.things:
            shifted = Thing(t.name, t.size, (t.start[0] + m, t.start[1] + m), t.path, t.seed, t.repaint)
            shifted.paste(big, f)
        dx, dy = (0, 0) if self.camera is None else self.camera[f]
        return np.ascontiguousarray(big[m - dy:m - dy + H, m - dx:m - dx + W])

    def frames(self, n):
        return np.stack([self.frame(f) for f in range(n)])

    def box(self, name, f):
        """The true box of thing `name` in frame f, the camera included."""
        t = next(t for t in self.things if t.name == name)
        dx, dy = (0, 0) if self.camera is None else self.camera[f]
        b = t.box(f)
        return [b[0] + dx, b[1] + dy, b[2], b[3]]


# what the named slots of the two streams are there for; (stream, slot in the first key record)
SLOTS = {'small': (0, 0), 'mid': (0, 1), 'flat': (0, 2), 'nan': (0, 3), 'zero': (0, 4),
         'large': (1, 0), 'big': (1, 1), 'painted': (1, 2), 'leaver': (1, 3)}
STEPS = {'small': (3, 2), 'mid': (-5, 4), 'large': (6, 1)}


@functools.lru_cache(maxsize=None)
def scenes():
    s0 = Scene(HW, 11, [Thing('small', (20, 20), (24, 22), STEPS['small'], 21),              # s = 1: min side <= 21 px
                        Thing('mid', (30, 36), (92, 30), STEPS['mid'], 22)],                 # s = 2
               flat=[(54, 86, 40, 40)])
    s1 = Scene(HW, 12, [Thing('large', (50, 56), (36, 34), STEPS['large'], 23),              # s = 3
                        Thing('painted', (20, 20), (100, 76), (0, 0), 24, repaint=(1,)),     # painted over in frame 1: lost
                        Thing('leaver', (16, 16), (126, 12), (1, 0), 25)])                   # its centre is at x = 128 in frame 2: left
    return s0, s1


def key_boxes(stream, f):
    """The boxes of the key record of frame f of a stream: the truth, and the slots that test the rules."""
    s0, s1 = scenes()
    if stream == 0:
        return [s0.box('small', f), s0.box('mid', f), [106, 74, 14, 14],                     # on the flat region
                [float('nan'), 10, 10, 10], [40, 80, 0, 12]]                                 # not carriable
    boxes = [s1.box('large', f), [64, 48, 400, 400], s1.box('painted', f)]                   # larger than the frame: s caps at 16
    return boxes + ([s1.box('leaver', f)] if f == 0 else [])


@functools.lru_cache(maxsize=None)
def rgb_frames():
    """uint8 [2, F, H, W, 3]."""
    return np.stack([sc.frames(F) for sc in scenes()])


def key_records(rot=False, frames=(0, 3)):
    """Per stream the int32 key records of the key frames `frames`."""
    out = []
    for s in range(2):
        rows = []
        for f in frames:
            boxes = key_boxes(s, f)
            rows.append(ref.record(boxes, angles=[0, 30, 45, 90, -20][:len(boxes)] if rot else None))
        out.append(rows)
    return out


def jump_scene():
    """One small box (s = 1, reach search * s = 4 pixels) that moves by (1, 1) per frame under a camera that jumps by (12, -9)."""
    camera = [(0, 0), (12, -9), (12, -9)]
    sc = Scene(HW, 31, [Thing('small', (20, 20), (50, 50), (1, 1), 32)], camera=camera)
    frames = sc.frames(3)[None]
    shift = np.array([[[0, 0, 0, 0], [12, -9, 1, 9], [0, 0, 1, 9]]], np.int64)
    return sc, frames, [[ref.record([sc.box('small', 0)])]], shift


REVERSAL_SETTINGS = dict(every=4, search=8, min_texture=1024, max_diff=24)


def reversal_scene():
    """An object that goes right for four frames and comes back fast for four, key frames at 0, 4 and 8."""
    path = [(3, 1)] * 4 + [(-8, -2)] * 4
    sc = Scene(HW, 41, [Thing('turner', (28, 28), (60, 44), path, 42)])
    frames = sc.frames(9)[None]
    return sc, frames, [[ref.record([sc.box('turner', f)], scores=[0.9], classes=[2]) for f in (0, 4, 8)]]
