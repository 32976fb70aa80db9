"""The cases of the appearance tests (test code): frames and boxes for the descriptor, hand-made records and descriptors for the
tracker.  tests/test_appear_host.py asserts the conditions the GPU tests rely on against the restatement alone."""
import numpy as np

H, W = 49, 67                                                        # RGB frames; the 4:2:0 ones are 48 x 66
TRACK_HW = (480, 640)


def frames(b=2, h=H, w=W, seed=5):
    """Noise in blocks of 3 x 2 pixels under a colour ramp: neighbouring pixels often fall into different bins."""
    rng = np.random.Generator(np.random.PCG64(seed))
    coarse = rng.integers(0, 256, size=(b, (h + 2) // 3, (w + 1) // 2, 3), dtype=np.uint8)
    img = np.repeat(np.repeat(coarse, 3, axis=1), 2, axis=2)[:, :h, :w].astype(np.int64)
    img[..., 0] += (np.arange(w) * 2)[None, None, :]
    return np.ascontiguousarray((img % 256).astype(np.uint8))


def named_rows():
    """The rows the issue names: (name, (cx, cy, w, h, angle))."""
    nan, inf = float('nan'), float('inf')
    return [('one_pixel', (20.5, 10.5, 1.0, 1.0, 0.0)), ('half_outside', (2.0, 24.0, 20.0, 30.0, 0.0)),
            ('outside', (-40.0, -30.0, 16.0, 24.0, 0.0)), ('angle_0', (33.3, 24.7, 18.0, 28.0, 0.0)),
            ('angle_30', (33.3, 24.7, 18.0, 28.0, 30.0)), ('angle_90', (33.3, 24.7, 18.0, 28.0, 90.0)),
            ('angle_-135', (30.1, 22.9, 17.0, 26.0, -135.0)), ('angle_450', (33.3, 24.7, 18.0, 28.0, 450.0)),
            ('nan', (nan, 20.0, 10.0, 10.0, 0.0)), ('inf', (30.0, 20.0, inf, 10.0, 0.0)), ('nan_angle', (30.0, 20.0, 10.0, 10.0, nan)),
            ('far_right', (80.0, 60.0, 12.0, 20.0, 180.0)), ('negative_w', (30.0, 20.0, -12.0, 20.0, 270.0))]


def boxes(k=24, seed=28):
    """float32 [2, k, 5] and counts int32 [2]: frame 0 the named rows and random rotated boxes, all k rows; frame 1 random
    boxes, axis-aligned, quarter-turned and rotated, of which the first k - 5 count."""
    rng = np.random.Generator(np.random.PCG64(seed))
    out = np.zeros((2, k, 5), np.float32)
    named = [r for _, r in named_rows()]
    out[0, :len(named)] = named
    for b, lo in ((0, len(named)), (1, 0)):
        for i in range(lo, k):
            kind = i % 3
            ang = (0.0, float(rng.choice([90.0, 180.0, 270.0, -90.0])), float(np.round(rng.uniform(-170, 170), 1)))[kind]
            out[b, i] = (rng.uniform(5, W - 5), rng.uniform(5, H - 5), rng.uniform(3, 40), rng.uniform(3, 40), ang)
    return out, np.array([k, k - 5], np.int32)


def tiny_boxes():
    """One frame of 512 tiny boxes (float32 [1, 512, 5]): the full count."""
    rng = np.random.Generator(np.random.PCG64(3))
    out = np.zeros((1, 512, 5), np.float32)
    out[0, :, 0], out[0, :, 1] = rng.uniform(0, W, 512), rng.uniform(0, H, 512)
    out[0, :, 2:4] = rng.uniform(0.5, 4.0, (512, 2))
    out[0, :, 4] = np.where(np.arange(512) % 2 == 0, 0.0, 90.0)
    return out


# ---- tracker ----

def flat(bins):
    """A descriptor uint16 [128] from {bin: count}."""
    d = np.zeros(128, np.uint16)
    for b, c in bins.items():
        d[b] = c
    return d


RED, BLUE, GREEN = flat({48: 256, 112: 256}), flat({3: 256, 67: 256}), flat({12: 256, 76: 256})
MIXED = flat({48: 128, 3: 128, 112: 128, 67: 128})                   # half RED, half BLUE: S = 65536 against either


def pack_desc(per_frame):
    """[[descriptor of record slot 0, 1, ...] per frame] -> uint16 [F, 512, 128]."""
    out = np.zeros((len(per_frame), 512, 128), np.uint16)
    for f, rows in enumerate(per_frame):
        for d, row in enumerate(rows):
            out[f, d] = row
    return out


def _fr(rows, width):
    """rows [(box5, score, cat)] -> a frame of _track_ref.pack_records."""
    if not rows:
        return (np.zeros((0, width), np.float32), np.zeros(0, np.float32), np.zeros(0, np.int64))
    return (np.array([r[0][:width] for r in rows], np.float32), np.array([r[1] for r in rows], np.float32), np.array([r[2] for r in rows], np.int64))


def lost_and_found(width=4, gap=4, jump=1.5):
    """Scenario (a): one object walks right for 4 frames, is missed for `gap` frames and returns `jump` box widths to the right of
    where its prediction is -- IoU 0 with it.  (frames, descs)."""
    w, h = 30.0, 50.0
    fr, ds = [], []
    x = 100.0
    for f in range(4):
        fr.append(_fr([((x + 4 * f, 200.0, w, h, 0.0), 0.9, 0)], width))
        ds.append([RED])
    for f in range(gap):
        fr.append(_fr([], width))
        ds.append([])
    back = x + 4 * (4 + gap) + jump * w                              # the prediction keeps walking at about 4 px per frame
    for f in range(3):
        fr.append(_fr([((back + 4 * f, 200.0, w, h, 0.0), 0.9, 0)], width))
        ds.append([RED])
    return fr, pack_desc(ds)


def crossing(width=4):
    """Scenario (b): two objects of one class side by side; in the last frame the better-scored detection (the BLUE object) has
    moved onto the RED track's prediction, and the RED object's detection lies between both predictions.  (frames, descs)."""
    w, h = 40.0, 60.0
    fr, ds = [], []
    for f in range(3):
        fr.append(_fr([((200.0, 200.0, w, h, 0.0), 0.9, 0), ((224.0, 200.0, w, h, 0.0), 0.8, 0)], width))
        ds.append([RED, BLUE])
    # record slot 0: the BLUE object, score 0.95, at x = 208: IoU 0.67 with RED's prediction (200), 0.43 with its own (224)
    # record slot 1: the RED object, score 0.7, at x = 214: IoU 0.48 with its own prediction, 0.6 with BLUE's
    fr.append(_fr([((208.0, 200.0, w, h, 0.0), 0.95, 0), ((214.0, 200.0, w, h, 0.0), 0.7, 0)], width))
    ds.append([BLUE, RED])
    return fr, pack_desc(ds)


def busy(width, n_frames=7, seed=2, bad=3, low=False, rot=False):
    """A scene for the == tests: 6 objects of two classes and three colours that drift, one of them missed for frames 2 .. 4 and
    back with a jump, one at a low score from frame 4 on (low=True), a bad-class frame at `bad`, a newcomer at frame 5.  (frames,
    descs); the descriptors carry a little per-frame variation so that templates blend."""
    rng = np.random.Generator(np.random.PCG64(seed))
    base = np.array([[100, 100, 30, 40, 10], [180, 110, 28, 44, 0], [260, 120, 32, 40, 170], [340, 300, 30, 42, 20], [420, 310, 26, 40, 0],
                     [500, 320, 30, 44, 5]], np.float64)
    if not rot:
        base[:, 4] = 0
    vel = np.array([[3, 1], [-2, 2], [2, -1], [1, 2], [-3, 0], [0, -2]], np.float64)
    cats = [0, 0, 1, 0, 1, 1]
    colours = [RED, BLUE, GREEN, MIXED, RED, BLUE]
    fr, ds = [], []
    for f in range(n_frames):
        if f == bad:
            fr.append(None)
            ds.append([])
            continue
        rows, drow = [], []
        for k in range(6):
            if k == 3 and 2 <= f <= 4:
                continue
            b = base[k].copy()
            b[:2] += vel[k] * f + ((55, 0) if k == 3 and f >= 5 else (0, 0))
            score = 0.9 - 0.05 * k
            if low and k == 1 and f >= 4:
                score = 0.4
            d = colours[k].copy().astype(np.int64)
            nz = np.flatnonzero(d)
            move = int(rng.integers(0, 40))
            d[nz[0]] -= move
            d[(nz[0] + 1 + f) % 128] += move
            rows.append((tuple(b), score, cats[k]))
            drow.append(d.astype(np.uint16))
        if f >= 5:
            rows.append(((60.0, 400.0, 30.0, 30.0, 0.0), 0.6, 0))
            drow.append(GREEN)
        fr.append(_fr(rows, width))
        ds.append(drow)
    return fr, pack_desc(ds)
