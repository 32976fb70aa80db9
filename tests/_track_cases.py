"""Hand-made association cases of the tracker, shared by tests/test_track_host.py (the numpy restatement against the
expectations written here) and tests/test_gpu_track.py (the kernel against the restatement).  Frames are 480 x 640.

A case: width (4 or 5), match, max_tracks, params (overrides of _track_ref.Params), frames = [(boxes, scores, cats) or None (a
bad-class frame)], expect = per frame {'id': [...], 'missed': [...], 'count', 'dropped'} over the max_tracks slots, pairs =
per frame the record slot each track slot matched or was born from (-1: neither), and `ties`, the number of deliberate
exact IoU ties.  Every IoU is at least 0.05 from match_thres, competing IoUs are 0.05 apart (except the ties) and every score
is 1e-3 from min_score and new_thres: the tests assert it on the float64 checker."""
import numpy as np

IMG_HW = (480, 640)


def _f(boxes, scores, cats=None):
    b = np.asarray(boxes, np.float32)
    b = b.reshape(len(scores), b.shape[-1])
    return b, np.asarray(scores, np.float32), np.asarray([0] * len(scores) if cats is None else cats, np.int64)


def _e(ids, missed, dropped=0, count=None):
    return {'id': ids, 'missed': missed, 'count': sum(i != 0 for i in ids) if count is None else count, 'dropped': dropped}


EMPTY = _f(np.zeros((0, 4)), [])


def full_case():
    """512 detections x 512 tracks: a 32 x 16 grid of 16 x 16 boxes 20 px apart, one class; frame 1 moves every box by 2 px
    (IoU 224 / 288 = 0.78 with its own track, 0 with every other) and shuffles the record order and the scores."""
    rng = np.random.Generator(np.random.PCG64(5))
    cx, cy = np.meshgrid(10 + 20 * np.arange(32), 10 + 20 * np.arange(16))
    base = np.stack([cx.ravel(), cy.ravel(), np.full(512, 16), np.full(512, 16)], axis=1).astype(np.float32)
    scores = np.linspace(0.9, 0.5, 512).astype(np.float32)
    s0 = scores[rng.permutation(512)]
    perm = rng.permutation(512)
    moved = base[perm] + np.array([2, 0, 0, 0], np.float32)
    s1 = scores[rng.permutation(512)]
    # frame 0: births in score order -> slot k holds the detection of rank k, id k + 1
    return dict(width=4, match='iou', max_tracks=512, params={}, ties=0,
                frames=[_f(base, s0), _f(moved, s1)],
                expect=[_e(list(range(1, 513)), [0] * 512), _e(list(range(1, 513)), [0] * 512)])


def cases():
    c = {}
    # the higher-scoring detection takes the track although the other overlaps it more (0.6 against 0.82); the loser is born
    c['two_detections_one_track'] = dict(width=4, match='iou', max_tracks=4, params={}, ties=0, frames=[
        _f([[100, 100, 40, 40]], [0.9]),
        _f([[104, 100, 40, 40], [110, 100, 40, 40]], [0.6, 0.8])],
        expect=[_e([1, 0, 0, 0], [0, -1, -1, -1]), _e([1, 2, 0, 0], [0, 0, -1, -1])], pairs=[[0, -1, -1, -1], [1, 0, -1, -1]])
    # one detection, two tracks: the larger IoU wins (0.74 against 0.48)
    c['two_tracks_one_detection'] = dict(width=4, match='iou', max_tracks=4, params={}, ties=0, frames=[
        _f([[100, 100, 40, 40], [120, 100, 40, 40]], [0.9, 0.8]),
        _f([[106, 100, 40, 40]], [0.7])],
        expect=[_e([1, 2, 0, 0], [0, 0, -1, -1]), _e([1, 2, 0, 0], [0, 1, -1, -1])], pairs=[[0, 1, -1, -1], [0, -1, -1, -1]])
    # ... and at exactly equal IoU (2/3 with both: integer coordinates) the lower slot, here the one with the LOWER score and
    # the HIGHER id: slot 0 is freed and refilled first
    c['exact_iou_tie'] = dict(width=4, match='iou', max_tracks=4, params={'max_missed': 1}, ties=1, frames=[
        _f([[400, 300, 40, 40], [116, 100, 40, 40]], [0.9, 0.8]),                # ids 1 (slot 0), 2 (slot 1)
        _f([[116, 100, 40, 40], [100, 100, 40, 40]], [0.8, 0.5]),                # slot 0 dies unmatched; id 3 is born into it
        _f([[108, 100, 40, 40]], [0.7])],
        expect=[_e([1, 2, 0, 0], [0, 0, -1, -1]), _e([3, 2, 0, 0], [0, 0, -1, -1]), _e([3, 0, 0, 0], [0, -1, -1, -1])],
        pairs=[[0, 1, -1, -1], [1, 0, -1, -1], [0, -1, -1, -1]])
    # the same place, another class: no match, a birth
    c['class_mismatch'] = dict(width=4, match='iou', max_tracks=4, params={}, ties=0, frames=[
        _f([[100, 100, 40, 40]], [0.9], [0]),
        _f([[100, 100, 40, 40]], [0.8], [1])],
        expect=[_e([1, 0, 0, 0], [0, -1, -1, -1]), _e([1, 2, 0, 0], [1, 0, -1, -1])], pairs=[[0, -1, -1, -1], [-1, 0, -1, -1]])
    # a frame with no detections, and a first frame with no tracks and no detections
    c['empty_frames'] = dict(width=4, match='iou', max_tracks=4, params={}, ties=0, frames=[
        EMPTY,
        _f([[100, 100, 40, 40], [300, 200, 60, 30]], [0.9, 0.8], [2, 5]),
        EMPTY,
        _f([[300, 200, 60, 30]], [0.6], [5])],
        expect=[_e([0, 0, 0, 0], [-1, -1, -1, -1]), _e([1, 2, 0, 0], [0, 0, -1, -1]), _e([1, 2, 0, 0], [1, 1, -1, -1]),
                _e([1, 2, 0, 0], [2, 0, -1, -1])], pairs=[[-1] * 4, [0, 1, -1, -1], [-1] * 4, [-1, 0, -1, -1]])
    # six births into four slots: the four best scores, in score order; two dropped; a detection below new_thres is neither
    c['six_births_four_slots'] = dict(width=4, match='iou', max_tracks=4, params={}, ties=0, frames=[
        _f([[50 + 90 * k, 100, 40, 40] for k in range(7)], [0.5, 0.9, 0.4, 0.7, 0.6, 0.8, 0.2])],
        expect=[_e([1, 2, 3, 4], [0, 0, 0, 0], dropped=2)], pairs=[[1, 5, 3, 4]])
    # a slot reused after a death, with a fresh id (max_missed 2; the birth happens in the frame of the death)
    c['slot_reuse'] = dict(width=4, match='iou', max_tracks=4, params={'max_missed': 2}, ties=0, frames=[
        _f([[100, 100, 40, 40], [300, 300, 40, 40]], [0.9, 0.8]),
        _f([[300, 300, 40, 40]], [0.8]),
        _f([[300, 300, 40, 40], [500, 200, 40, 40]], [0.8, 0.7])],
        expect=[_e([1, 2, 0, 0], [0, 0, -1, -1]), _e([1, 2, 0, 0], [1, 0, -1, -1]), _e([3, 2, 0, 0], [0, 0, -1, -1])],
        pairs=[[0, 1, -1, -1], [-1, 0, -1, -1], [1, 0, -1, -1]])
    # a bad-class frame changes nothing: the track is matched in the next frame after ONE prediction
    c['bad_class_frame'] = dict(width=4, match='iou', max_tracks=4, params={}, ties=0, frames=[
        _f([[100, 100, 40, 40]], [0.9]),
        None,
        _f([[102, 100, 40, 40]], [0.8])],
        expect=[_e([1, 0, 0, 0], [0, -1, -1, -1]), _e([0, 0, 0, 0], [-1, -1, -1, -1], count=-1), _e([1, 0, 0, 0], [0, -1, -1, -1])],
        pairs=[[0, -1, -1, -1], [-1] * 4, [0, -1, -1, -1]])
    # the angle wrap: a track at 179 degrees takes a detection at 1 degree (the same bar turned by 2 degrees)
    c['angle_wrap'] = dict(width=5, match='rotated', max_tracks=4, params={}, ties=0, frames=[
        _f([[200, 200, 80, 30, 179]], [0.9]),
        _f([[200, 200, 80, 30, 1]], [0.8]),
        _f([[200, 200, 80, 30, 178]], [0.8])],
        expect=[_e([1, 0, 0, 0], [0, -1, -1, -1])] * 3, pairs=[[0, -1, -1, -1]] * 3)
    # two crossed bars with one centre: the rotated test gives the detection to the bar of its own direction (IoU 0.11 with
    # the other); the axis-aligned test on (cx, cy, w, h) sees two identical boxes -- a tie, the lower slot
    crossed = [_f([[200, 200, 100, 20, 0], [200, 200, 100, 20, 90]], [0.9, 0.8]), _f([[200, 200, 100, 20, 88]], [0.7])]
    c['rotated_match'] = dict(width=5, match='rotated', max_tracks=4, params={}, ties=0, frames=crossed,
                              expect=[_e([1, 2, 0, 0], [0, 0, -1, -1]), _e([1, 2, 0, 0], [1, 0, -1, -1])],
                              pairs=[[0, 1, -1, -1], [-1, 0, -1, -1]])
    c['iou_match_on_rotated_records'] = dict(width=5, match='iou', max_tracks=4, params={}, ties=1, frames=crossed,
                                             expect=[_e([1, 2, 0, 0], [0, 0, -1, -1]), _e([1, 2, 0, 0], [0, 1, -1, -1])],
                                             pairs=[[0, 1, -1, -1], [0, -1, -1, -1]])
    return c
