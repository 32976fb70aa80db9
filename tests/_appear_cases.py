"""The cases of the appearance tests (test code): frames and boxes for the descriptor, hand-made records and descriptors for the
tracker, and the branch cases of tests/test_gpu_appear_branches.py.  tests/test_appear_host.py asserts the conditions the GPU tests rely on against the restatement alone."""
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


# ---- the branch cases (tests/test_gpu_appear_branches.py; tests/test_appear_host.py proves each on the restatement alone) ----
#
# A tracker case is a dict: frames, descs (as above), width, match, mt, params (of track_params), assoc (of track_assoc, or None),
# shifts (int32 [F, 4] or None), appear -- gate and reid as RAW integers on the scale of S, alpha, reach, update_thres, the
# keywords of _appear_ref.Stream and the fields of the mydet_track_appear struct -- and expect: [(frame, slot, how)], the
# outcomes the case is for.

BANDS = dict(low_thres=0.2, high_thres=0.5, low_match_thres=0.3)
BOX = (200.0, 200.0, 40.0, 60.0, 0.0)
ONE, ZERO, TWO = flat({5: 512}), flat({}), flat({5: 100, 9: 300, 77: 111, 20: 1})          # one bin holds every sample; an all-zero row
TEMPLATE_SEQ = [ONE, ZERO] * 3 + [ONE, TWO, TWO] * 2
SIM_MAX = 131072


def level(v):
    """ops.appear_set's integer level of a fraction."""
    return int(np.floor(v * SIM_MAX + 0.5))


def up(v):
    """One float32 step above v."""
    return float(np.nextafter(np.float32(v), np.float32(np.inf)))


def case(frames, per_frame_descs, expect=(), **kw):
    c = dict(frames=frames, descs=per_frame_descs if isinstance(per_frame_descs, np.ndarray) else pack_desc(per_frame_descs), width=4,
             match='iou', mt=64, params={}, assoc=None, shifts=None, expect=list(expect))
    c['appear'] = dict(dict(gate=0, reid=0, alpha=26, reach=2.0, update_thres=0.3), **kw.pop('appear', {}))
    c.update(kw)
    return c


def restate(c, cls=None, **over):
    """A case through the restatement (or a subclass of its Stream), `over` replacing appearance settings: _appear_ref.run's
    (stream, outs, arrays)."""
    import _appear_ref
    import _track_ref
    par = _track_ref.Params(TRACK_HW, np.float32, match=c['match'], **c['params'])
    stream = (cls or _appear_ref.Stream)(c['mt'], par, **dict(c['appear'], **over), **(c['assoc'] or {}))
    return _appear_ref.run(c['frames'], c['descs'], c['width'], TRACK_HW, c['mt'], shifts=c['shifts'], stream=stream)


def _row(box=BOX, score=0.9, cat=0):
    return (tuple(float(v) for v in box), score, cat)


def _f(*rows):
    return _fr(list(rows), 4)


def pad_scene(scene, n):
    """A (frames, descs) scene padded to n frames with empty ones."""
    fr, ds = scene
    width = 4 if fr[0] is None or fr[0][0].shape[1] == 4 else 5
    return fr + [_fr([], width)] * (n - len(fr)), np.concatenate([ds, np.zeros((n - len(ds), 512, 128), np.uint16)])


def stream_scenes(width=4, low=False, rot=False):
    """Three streams with a scene each -- busy, lost_and_found, crossing -- padded to a common F."""
    scenes = [busy(width, low=low, rot=rot), lost_and_found(width), crossing(width)]
    n = max(len(s[0]) for s in scenes)
    return [pad_scene(s, n) for s in scenes]


# -- many detections --
MANY_N, MANY_LOST, MANY_STRANGER, MANY_FRAME = 150, (3, 70, 135), 100, 4


def many_desc(i, f):
    """The descriptor of object i in frame f: three bins of its own, a little of it moving with the frame."""
    d = np.zeros(128, np.uint16)
    b = i % 128
    d[b], d[(b + 64) % 128], d[(b + 37) % 128] = 312 - 8 * f, 8 * f, 200
    return d


def many(mt=192):
    """150 objects on a 15 x 10 grid of 20 x 24 boxes, 40 x 44 apart, scores falling with the index (rank = index = slot of
    birth).  Objects 3, 70, 135 and 100 are absent in frames 2 and 3 and return in frame 4 displaced by (20, 22) -- IoU 0 with
    every prediction, within reach 2 * 24 -- at the lowest scores of the frame; 100 returns with another descriptor.  Two
    newcomers out of every lost track's reach, at scores 0.99 and 0.80, put candidates into the first two words of the mask."""
    pos = [(30.0 + 40.0 * (i % 15), 30.0 + 44.0 * (i // 15)) for i in range(MANY_N)]
    gone = MANY_LOST + (MANY_STRANGER,)
    frames, descs = [], []
    for f in range(6):
        rows, drow = [], []
        for i in range(MANY_N):
            if i in gone and f >= 2:
                continue
            rows.append(_row((pos[i][0], pos[i][1], 20.0, 24.0, 0.0), 0.95 - 0.002 * i))
            drow.append(many_desc(i, f))
        if f >= MANY_FRAME:
            for k, i in enumerate(gone):
                rows.append(_row((pos[i][0] + 20.0, pos[i][1] + 22.0, 20.0, 24.0, 0.0), 0.5 - 0.01 * k))
                drow.append(many_desc(i + 11 if i == MANY_STRANGER else i, f))
            for k, (x, score) in enumerate(((610.0, 0.99), (570.0, 0.80))):
                rows.append(_row((x, 462.0, 20.0, 24.0, 0.0), score))
                drow.append(many_desc(200 + 5 * k, f))
        frames.append(_f(*rows))
        descs.append(drow)
    expect = [(MANY_FRAME, s, 3) for s in MANY_LOST if s < mt]
    if mt >= MANY_N + 3:
        expect += [(MANY_FRAME, MANY_STRANGER, 0)] + [(MANY_FRAME, MANY_N + k, 4) for k in range(3)]
    return case(frames, descs, expect, mt=mt, appear=dict(gate=level(0.3), reid=level(0.6)))


# -- the integer levels at equality: S(RED template, MIXED) = 65536 exactly --
def threshold_cases():
    far = (260.0, 200.0, 40.0, 60.0, 0.0)
    out = {}
    for lv, ok in ((65536, True), (65537, False)):
        out[f'gate_high_{lv}'] = case([_f(_row())] * 2, [[RED], [MIXED]], [(1, 0, 1), (1, 1, -1)] if ok else [(1, 0, 0), (1, 1, 4)],
                                      appear=dict(gate=lv))
        out[f'gate_low_{lv}'] = case([_f(_row()), _f(_row(score=0.4))], [[RED], [MIXED]], [(1, 0, 2 if ok else 0), (1, 1, -1)],
                                     appear=dict(gate=lv), assoc=BANDS)
        out[f'reid_{lv}'] = case([_f(_row())] * 2 + [_f()] * 2 + [_f(_row(far))], [[RED], [RED], [], [], [MIXED]],
                                 [(4, 0, 3), (4, 1, -1)] if ok else [(4, 0, 0), (4, 1, 4)], appear=dict(reid=lv))
    return out


# -- the gate changes the outcome --
def gate_cases():
    two = [_f(_row(), _row((224.0, 200.0, 40.0, 60.0, 0.0), 0.8))] * 3
    at208 = _f(_row((208.0, 200.0, 40.0, 60.0, 0.0), 0.95))            # IoU 0.67 with slot 0 (RED), 0.43 with slot 1 (BLUE)
    return {
        'second_takes': case(two + [at208], [[RED, BLUE]] * 3 + [[BLUE]], [(3, 0, 0), (3, 1, 1)], appear=dict(gate=level(0.3))),
        'all_refuse': case(two + [at208], [[RED, BLUE]] * 3 + [[GREEN]], [(3, 0, 0), (3, 1, 0), (3, 2, 4)], appear=dict(gate=level(0.3))),
        'walk_refuses_reid_takes': case([_f(_row())] * 2 + [_f()] * 2 + [_f(_row())], [[RED], [RED], [], [], [MIXED]], [(4, 0, 3), (4, 1, -1)],
                                        appear=dict(gate=level(0.6), reid=level(0.4))),
    }


# -- the guards of the re-identification: each case changes one thing against the base beside it --
def guard_cases():
    far = (260.0, 200.0, 40.0, 60.0, 0.0)

    def g(gap, back, expect, **kw):
        n = 2 + gap
        return case([_f(_row())] * 2 + [_f()] * gap + [_f(back)], [[RED], [RED]] + [[]] * gap + [[RED]], [(n, s, h) for s, h in expect],
                    appear=dict(reid=level(0.5)), **kw)
    return {
        'base': g(1, _row(far), [(0, 3), (1, -1)]),
        'gap_0': g(0, _row(far), [(0, 0), (1, 4)]),
        'other_class': g(1, _row(far, cat=1), [(0, 0), (1, 4)]),
        'below_new_thres': g(1, _row(far, score=0.25), [(0, 0), (1, -1)]),
        'bands_base': g(1, _row(far), [(0, 3), (1, -1)], assoc=BANDS),
        'low_band': g(1, _row(far, score=0.4), [(0, 0), (1, -1)], assoc=BANDS),
    }


# -- reach: the tracks stand still, so the prediction is the born box exactly; reach 1.5 * 80 = 120 px --
REACH_SIZES = {'track_w': ((80.0, 40.0), (30.0, 50.0)), 'track_h': ((40.0, 80.0), (50.0, 30.0)),
               'det_w': ((30.0, 50.0), (80.0, 40.0)), 'det_h': ((50.0, 30.0), (40.0, 80.0))}


def reach_cases():
    """name -> case; '<x>_at' lies on the bound (found, how 3), '<x>_past' one float32 step beyond (born, how 4)."""
    out = {}
    found, born = [(4, 0, 3), (4, 1, -1)], [(4, 0, 0), (4, 1, 4)]

    def r(track, det, cx, cy, expect, shifts=None, **appear):
        t = _row((200.0, 200.0, track[0], track[1], 0.0))
        return case([_f(t)] * 2 + [_f()] * 2 + [_f(_row((cx, cy, det[0], det[1], 0.0)))], [[RED], [RED], [], [], [RED]], expect, shifts=shifts,
                    appear=dict(dict(reid=level(0.5), reach=1.5), **appear))
    for name, (track, det) in REACH_SIZES.items():
        out[name + '_at'], out[name + '_past'] = r(track, det, 320.0, 200.0, found), r(track, det, up(320.0), 200.0, born)
    track, det = REACH_SIZES['track_w']
    out['y_only_at'], out['y_only_past'] = r(track, det, 200.0, 320.0, found), r(track, det, 200.0, up(320.0), born)
    # reach 0: only a coincident centre; the walk refuses the pair (reid <= S < gate), so the re-identification sees it
    lv = dict(gate=level(0.6), reid=level(0.4), reach=0.0)
    for name, cx, expect in (('reach_0_at', 200.0, found), ('reach_0_past', up(200.0), born)):
        out[name] = case([_f(_row())] * 2 + [_f()] * 2 + [_f(_row((cx, 200.0, 40.0, 60.0, 0.0)))], [[RED], [RED], [], [], [MIXED]], expect,
                         appear=dict(dict(alpha=26, update_thres=0.3), **lv))
    # a valid camera shift in the frame of the return: the distance is measured from the shifted prediction (207, 197)
    shifts = np.zeros((5, 4), np.int32)
    shifts[4] = (7, -3, 1, 9)
    out['shift_at'], out['shift_past'] = r(track, det, 327.0, 197.0, found, shifts), r(track, det, up(327.0), 197.0, born, shifts)
    return out


# -- template arithmetic: one track, one frame per launch --
def template_cases():
    seq = TEMPLATE_SEQ
    frames = [_f(_row())] * len(seq)
    return {
        'alpha_1': case(frames, [[d] for d in seq], [(f, 0, 1) for f in range(1, len(seq))], appear=dict(alpha=1)),
        'alpha_256': case(frames, [[d] for d in seq], [(f, 0, 1) for f in range(1, len(seq))], appear=dict(alpha=256)),
        # the gate on and a template present: the zero row has S = 0 and is refused (and born: a template of zeros)
        'zero_refused': case([_f(_row())] * 3, [[ONE], [ZERO], [ONE]], [(1, 0, 0), (1, 1, 4), (2, 0, 1), (2, 1, 0)], appear=dict(gate=level(0.3))),
    }


def retire_rebirth():
    """The match of frame 1 carries track 1 beyond the right border (x[0] > 640): it is retired, and the unmatched BLUE detection
    is born into its slot in the same frame."""
    return case([_f(_row((635.0, 200.0, 40.0, 60.0, 0.0))), _f(_row((650.0, 200.0, 40.0, 60.0, 0.0)), _row((100.0, 100.0, 40.0, 60.0, 0.0), 0.8))],
                [[RED], [RED, BLUE]], [(1, 0, 4), (1, 1, -1)])


# -- descriptor --
P29 = 2.0 ** 29


def ragged_boxes(k, seed=41, h=48, w=66):
    """float32 [2, k, 5]: axis-aligned and quarter-turned boxes (every one settled)."""
    rng = np.random.Generator(np.random.PCG64(seed + k))
    out = np.zeros((2, k, 5), np.float32)
    for b in range(2):
        for i in range(k):
            ang = 0.0 if (i + b) % 2 == 0 else float(rng.choice([90.0, 180.0, 270.0, -90.0]))
            out[b, i] = (rng.uniform(2, w - 2), rng.uniform(2, h - 2), rng.uniform(3, 40), rng.uniform(3, 40), ang)
    return out


def edge_frames():
    """Frames of one row, of one column and of one pixel."""
    return {'h1': frames(2, 1, W, seed=6), 'w1': frames(2, H, 1, seed=7), '1x1': frames(2, 1, 1, seed=8)}


def edge_boxes():
    """float32 [2, 6, 5] for the frames of edge_frames: inside, outside, larger than the frame, quarter-turned, zero size."""
    rows = [(0.5, 0.5, 1.0, 1.0, 0.0), (30.2, 20.7, 18.0, 28.0, 0.0), (-9.0, 60.0, 12.0, 20.0, 90.0), (33.3, 24.7, 300.0, 200.0, 180.0),
            (20.5, 10.5, 0.0, 0.0, 0.0), (3.0, 2.0, 7.0, 90.0, 270.0)]
    return np.array([rows, rows[::-1]], np.float32)


def bound_rows():
    """(name, row) around the 2^29 bound, for the 49 x 67 frames.  at_*: a box of zero size on the bound, all 512 taps counted and
    clamped to the border; past_*: one float32 step beyond, a box that sums to 0; half*: w = 4096 centred on the bound, the
    columns on one side beyond it (the float32 spacing there is 64)."""
    p, q = P29, up(P29)
    return [('zero_size', (20.5, 10.5, 0.0, 0.0, 0.0)), ('zero_size_90', (40.2, 30.9, 0.0, 0.0, 90.0)),
            ('at_+x', (p, 20.0, 0.0, 0.0, 0.0)), ('at_-x', (-p, 20.0, 0.0, 0.0, 0.0)), ('at_+y', (30.0, p, 0.0, 0.0, 0.0)),
            ('at_-y', (30.0, -p, 0.0, 0.0, 0.0)), ('past_+x', (q, 20.0, 0.0, 0.0, 0.0)), ('past_-x', (-q, 20.0, 0.0, 0.0, 0.0)),
            ('past_+y', (30.0, q, 0.0, 0.0, 0.0)), ('past_-y', (30.0, -q, 0.0, 0.0, 0.0)), ('half', (p, 20.0, 4096.0, 10.0, 0.0)),
            ('half_180', (p, 20.0, 4096.0, 10.0, 180.0)), ('half_-y', (30.0, -p, 10.0, 8192.0, 0.0))]


def bound_boxes():
    """float32 [2, 13, 5]: the rows of bound_rows, in frame 1 in reverse order."""
    rows = [r for _, r in bound_rows()]
    return np.array([rows, rows[::-1]], np.float32)
