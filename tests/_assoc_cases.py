"""Hand-made cases of the tracker's association modes (include/mydet.h: mydet_track_assoc), shared by tests/test_assoc_host.py
(the float64 restatement against the expectations written here, with its margins) and tests/test_gpu_assoc.py (the kernel against
the restatement).  Frames are 480 x 640, every box is integer-valued.

A case: width, match, max_tracks, params (overrides of _track_ref.Params), assoc (the keyword arguments of _assoc_ref.Stream and
ops.track_assoc), frames = [(boxes, scores, cats) or None], expect = per frame {'id', 'missed', 'count', 'dropped'} or None where
the float64 restatement is the expectation (the large case), ties = the deliberate exact ties.  Every IoU is at least 0.05 from
its stage's threshold, every score 1e-3 from the thresholds it is compared with, and the optimal total is 0.05 * 65536 from the
total of every other pairing (except the ties): the tests assert it on the float64 restatement."""
import numpy as np

from _track_cases import IMG_HW, _e, _f            # noqa: F401  (IMG_HW is re-exported)

BANDS = dict(low_thres=0.1, high_thres=0.3, low_match_thres=0.3)


def _with_angle(boxes, turn):
    """4-wide integer boxes as 5-wide ones: angle 0, or (turn) the same rectangle written as (cx, cy, h, w, 90)."""
    b = np.asarray(boxes, np.float32)
    if turn:
        return np.stack([b[:, 0], b[:, 1], b[:, 3], b[:, 2], np.full(len(b), 90, np.float32)], axis=1)
    return np.concatenate([b, np.zeros((len(b), 1), np.float32)], axis=1)


def ab_case(variant, assign):
    """The example of the rules, 40 x 30 boxes: A (score 0.85) has IoU 0.6 with track 1 and 0.5 with track 2, B (0.7) has 0.574
    with track 1 and 0.185 with track 2.  Greedy: A takes track 1, B is born as id 3 and track 2 coasts.  Optimal: A takes
    track 2 and B track 1 (total 1.074 against 0.6 + nothing).  variant: '4', '5iou' or '5rot' (the detections of frame 1 are
    written at 90 degrees: the same rectangles)."""
    t = [[100, 100, 40, 30], [110, 110, 40, 30]]
    d = [[110, 100, 40, 30], [95, 95, 40, 30]]
    if variant == '4':
        f0, f1, width, match = t, d, 4, 'iou'
    else:
        f0, f1, width, match = _with_angle(t, False), _with_angle(d, variant == '5rot'), 5, 'rotated' if variant == '5rot' else 'iou'
    expect = [_e([1, 2, 0, 0], [0, 0, -1, -1])]
    expect.append(_e([1, 2, 0, 0], [0, 0, -1, -1]) if assign == 'optimal' else _e([1, 2, 3, 0], [0, 1, 0, -1]))
    return dict(width=width, match=match, max_tracks=4, params={}, assoc=dict(assign=assign), ties=0,
                frames=[_f(f0, [0.9, 0.8]), _f(f1, [0.85, 0.7])], expect=expect)


P1, P2, P3, FAR = [100, 100, 40, 40], [300, 100, 40, 40], [500, 100, 40, 40], [100, 300, 40, 40]


def bands_frames():
    """Three still objects (conf_thres 0.3, low_thres 0.1).  Track 1 is matched for three frames, gets a 0.2 detection in
    frames 3 and 4 and a high one in frame 5.  Beside it: frame 1 a low detection on track 1, which a high one already took
    (never offered to stage 2, never born); frame 2 a low detection far from everything (never born); frame 3 nothing for track
    2 and a 0.05 detection on track 3 (ignored); frame 4 low detections on tracks 2 and 3, which have missed == 2 by then (not
    continued)."""
    return [_f([P1, P2, P3], [0.9, 0.8, 0.7]),
            _f([P1, [104, 100, 40, 40], P2, P3], [0.9, 0.2, 0.8, 0.7]),
            _f([P1, P2, P3, FAR], [0.9, 0.8, 0.7, 0.2]),
            _f([P1, P3], [0.2, 0.05]),
            _f([P1, P2, P3], [0.2, 0.2, 0.2]),
            _f([P1, P2, P3], [0.9, 0.8, 0.7])]


def _filtered(frames, thres):
    out = []
    for b, s, c in frames:
        keep = s >= np.float32(thres)
        out.append((b[keep], s[keep], c[keep]))
    return out


def bands_case(assign, bands=True):
    """bands=False: the same records as a post-process at 0.3 leaves them, and one band: the tracks coast."""
    ids = [1, 2, 3, 0, 0, 0, 0, 0]
    missed = [[0, 0, 0], [0, 0, 0], [0, 0, 0], [0, 1, 1], [0, 2, 2], [0, 0, 0]] if bands else \
             [[0, 0, 0], [0, 0, 0], [0, 0, 0], [1, 1, 1], [2, 2, 2], [0, 0, 0]]
    frames = bands_frames()
    return dict(width=4, match='iou', max_tracks=8, params={}, assoc=dict(assign=assign, **(BANDS if bands else {})), ties=0,
                frames=frames if bands else _filtered(frames, 0.3), expect=[_e(ids, m + [-1] * 5) for m in missed])


def classes_case(assign):
    """Two classes interleaved in slot order.  Every detection overlaps the track of the OTHER class more (0.739) than its own
    (0.481): an assignment that ignored classes would cross all four."""
    t = [[100, 100, 40, 40], [120, 100, 40, 40], [300, 100, 40, 40], [320, 100, 40, 40]]
    d = [[114, 100, 40, 40], [106, 100, 40, 40], [314, 100, 40, 40], [306, 100, 40, 40]]
    return dict(width=4, match='iou', max_tracks=4, params={}, assoc=dict(assign=assign), ties=0,
                frames=[_f(t, [0.9, 0.8, 0.7, 0.6], [0, 1, 0, 1]), _f(d, [0.5, 0.8, 0.6, 0.7], [0, 1, 0, 1])],
                expect=[_e([1, 2, 3, 4], [0, 0, 0, 0])] * 2)


def tie_case(assign, variant='4'):
    """Two tracks that mirror each other about the detection: bit-equal IoU 2/3, the lower slot takes it."""
    t, d = [[116, 100, 40, 40], [100, 100, 40, 40]], [[108, 100, 40, 40]]
    width, match = (4, 'iou') if variant == '4' else (5, 'rotated')
    if width == 5:
        t, d = _with_angle(t, False), _with_angle(d, False)
    return dict(width=width, match=match, max_tracks=4, params={}, assoc=dict(assign=assign), ties=1,
                frames=[_f(t, [0.9, 0.8]), _f(d, [0.7])], expect=[_e([1, 2, 0, 0], [0, 0, -1, -1]), _e([1, 2, 0, 0], [0, 1, -1, -1])])


def bad_class_case(assoc):
    return dict(width=4, match='iou', max_tracks=4, params={}, assoc=assoc, ties=0,
                frames=[_f([[100, 100, 40, 40]], [0.9]), None, _f([[102, 100, 40, 40]], [0.8])],
                expect=[_e([1, 0, 0, 0], [0, -1, -1, -1]), _e([0, 0, 0, 0], [-1, -1, -1, -1], count=-1), _e([1, 0, 0, 0], [0, -1, -1, -1])])


GRID_MT, GRID_DETS = 130, 70
# a measurement noise so large that a matched track stays where it is (gain 1e-4): frame 3 meets the tracks on the grid again
GRID_PARAMS = dict(match_thres=0.06, r=(10, 10, 10, 10, 100))
# (gap k, offset) of a grid row's seven detections.  A detection in gap k at offset o overlaps track k and track k + 1 only, with
# IoU (left / right) 0.583 / 0.118 at o = 10, 0.462 / 0.188 at 14, 0.357 / 0.267 at 18, and the mirror images at 30, 26:
#   a pair   (0, 30) (1, 14): both want track 1; best is 0 -> 1, 1 -> 2 (0.771 against 0.583 and 0.580)
#   a chain  (3, 26) (4, 14) (5, 14): best is every detection on its LEFT track (1.111 against 0.923 with the middle one
#            unmatched); a greedy walk that meets the first one first sends all three to the right
#   a triple (3, 10) (3, 30) (3, 18): three detections for two tracks, the third ends on its dummy column
#   singles  (7, 10) (9, 26)
GRID_ROW_A = [(0, 30), (1, 14), (3, 26), (4, 14), (5, 14), (7, 10), (9, 26)]
GRID_ROW_B = [(11 - k, 40 - o) for k, o in [(0, 30), (1, 14), (3, 10), (3, 30), (3, 18), (7, 10), (9, 26)]]


def grid_frames(seed):
    """Four frames for 130 track slots (three wavefronts).  Frames 0 and 1 fill the slots: 65 boxes each, 36 x 20 on a 13 x 10
    grid with 40 px spacing (the even and then the odd grid rows, so no box overlaps another), born in score order, so the
    slots are not in grid order.  Frames 2 and 3 hold 70 detections each, 40 x 20, seven per grid row in the patterns above (A
    on the even rows and B on the odd ones, then the other way round): every detection overlaps exactly two neighbouring
    tracks.  Scores and record slots are shuffled.  With 130 live tracks the five unmatched detections of a frame find no
    free slot: they are counted as dropped."""
    rng = np.random.Generator(np.random.PCG64(seed))
    frames = []
    for parity in (0, 1):
        b = [[30 + 40 * i, 30 + 40 * j, 36, 20] for j in range(parity, 10, 2) for i in range(13)]
        frames.append(_f(b, np.linspace(0.95, 0.6, len(b))[rng.permutation(len(b))]))
    for swap in (0, 1):
        b = [[30 + 40 * k + o, 30 + 40 * j, 40, 20] for j in range(10) for k, o in (GRID_ROW_A if (j + swap) % 2 == 0 else GRID_ROW_B)]
        b = np.asarray(b)[rng.permutation(GRID_DETS)]
        frames.append(_f(b, np.linspace(0.9, 0.4, GRID_DETS)[rng.permutation(GRID_DETS)]))
    return frames


def crossing():
    """Twelve frames of two 40 x 30 objects of one class that pass close by each other, as (records per frame, ground-truth boxes
    per frame).  Frames 0-4: object 1 at (100, 100), object 2 at (110, 110).  From frame 5 on they stand at (95, 95) and
    (110, 100): the configuration of ab_case, in which the greedy walk gives object 2 (the higher score) the track of object
    1.  Object 1 scores 0.2 in frames 8 and 9, below a conf_thres of 0.3."""
    frames, truth = [], []
    for f in range(12):
        o1, o2 = ([100, 100, 40, 30], [110, 110, 40, 30]) if f < 5 else ([95, 95, 40, 30], [110, 100, 40, 30])
        frames.append(_f([o1, o2], [0.2 if f in (8, 9) else 0.7, 0.85]))
        truth.append([o1, o2])
    return frames, truth
