"""GPU tests of the tracker with the similarity model (include/mydet.h: mydet_track_frames_warp_f32 and its two appearance
siblings; csrc/track.hip: the warp branch of `predict`), and of the model through the Detector.

The checker of the predict step is tests/_warp_ref.py: every line one rounded float32 operation, so outputs and state agree bit
for bit.  The appearance entry points are held to the same restatement with their gate, re-identification and weight off, where
include/mydet.h makes their tracker outputs and state those of the plain entry point."""
import math

import numpy as np
import pytest
import torch

import _assoc_ref as aref
import _motion_ref as mref
import _track_ref
import _warp_ref as ref
from test_gpu_track import _assert_state_equals, _bits

pytestmark = pytest.mark.gpu

HW = (480, 640)
MT = 64
# the camera of frame f > 0: (degrees, zoom, shift); frame 3 reports nothing (valid 0) and the camera rests; frame 5 is a
# bad-class frame whose row is valid all the same
CAMERA = [None, (1.5, 1.02, (6.25, -4.5)), (-2.0, 0.98, (-5.0, 3.75)), None, (0.75, 1.0, (0.0, 0.0)), (1.0, 1.01, (2.0, 2.0)),
          (0.0, 1.03, (-3.5, 0.0)), (-1.25, 1.0, (4.0, -7.0))]
BAD_FRAME = 5
OPTIMAL_BANDS = dict(assign='optimal', low_thres=0.3, high_thres=0.6, low_match_thres=0.3)


def warp_row(deg, zoom, shift, n=9):
    """A valid warp row of a true camera step, as the estimator would report it."""
    a, b, tx, ty = (int(round(v * 65536)) for v in ref.true_model(deg, zoom, shift))
    s_q, deg_q = ref.derived(a, b, ref.Fit(max_zoom=0.25, max_rotation=14.0))
    return [a, b, tx, ty, s_q, deg_q, 1, n]


def scenario(width, low_from=None):
    """Three boxes of about 24 px that drift slowly in the world while the camera turns, zooms and shifts: the records are the
    boxes under the accumulated camera.  Returns (frames for pack_records, warp rows int32 [F, 8])."""
    base = np.array([[200.0, 150.0, 24.0, 26.0, 10.0], [330.0, 250.0, 22.0, 24.0, 0.0], [440.0, 330.0, 26.0, 24.0, 170.0]])
    drift = np.array([[1.0, 0.5], [-0.5, 1.0], [0.75, -0.75]])
    cats = np.array([0, 0, 1], np.int64)
    rows = np.zeros((len(CAMERA), 8), np.int32)
    cur = base.copy()
    frames = []
    for f, cam in enumerate(CAMERA):
        if cam is not None:
            rows[f] = warp_row(*cam)
        if f == BAD_FRAME:                                           # the camera of a bad-class frame is not applied to the world
            frames.append(None)
            continue
        cur[:, :2] += drift
        if cam is not None:
            deg, zoom, _ = cam
            cur[:, 0], cur[:, 1] = ref.apply_model(ref.true_model(*cam), HW, cur[:, 0].copy(), cur[:, 1].copy())
            cur[:, 2:4] *= zoom
            cur[:, 4] = (cur[:, 4] + deg) % 180.0
        scores = np.array([0.9, 0.8, 0.45 if low_from is not None and f >= low_from else 0.7], np.float32)
        frames.append((cur[:, :width].astype(np.float32), scores, cats))
    return frames, rows


def _launch(rec, rows, par, family, assoc, cuts, width, shifts=None):
    """The records through one entry-point family on fresh states: the outputs [F, ...] as numpy and the tracker state.  rows:
    warp rows [F, 8] or None; shifts: shift rows [F, 4] in their place."""
    from mydetection_amd import ops
    F = rec.shape[0]
    state = ops.track_state(1, MT, 'cuda')
    kw = {}
    if family.startswith('appear'):
        desc = torch.zeros((F, 512, 128), dtype=torch.uint16, device='cuda')
        astate = ops.appear_state(1, MT, 'cuda')
        aset = ops.appear_set(gate=None, reid=None)
        if family == 'appear_optimal':
            kw.update(appear_weight=0, appear_ws=ops.appear_workspace(1, MT, 'cuda'))
    outs, lo = [], 0
    for n in cuts:
        if family.startswith('appear'):
            kw['appear'] = (aset, desc[lo:lo + n].contiguous(), astate)
        w = None if rows is None else torch.from_numpy(rows[lo:lo + n]).cuda().view(1, n, 8)
        sh = None if shifts is None else torch.from_numpy(shifts[lo:lo + n]).cuda().view(1, n, 4)
        outs.append(ops.track_frames(rec[lo:lo + n], state, par, assoc=assoc, warp=w, shift=sh, **kw))
        lo += n
    return {k: torch.cat([o[k] for o in outs], dim=1)[0].cpu().numpy() for k in ('box', 'score', 'id', 'missed', 'count', 'dropped')}, state


FAMILIES = {'plain': None, 'assoc': OPTIMAL_BANDS, 'appear': None, 'appear_optimal': dict(assign='optimal')}


@pytest.mark.parametrize('width', (4, 5))
@pytest.mark.parametrize('family', sorted(FAMILIES))
def test_the_predict_step_equals_the_float32_restatement(family, width):
    """Outputs and state bit for bit, in one launch and in two, with an invalid row and a bad-class frame on the way; the
    ids persist, which they do not on the same records without the rows."""
    from mydetection_amd import ops
    assoc = FAMILIES[family]
    frames, rows = scenario(width, low_from=3 if family == 'assoc' else None)
    s64, o64, _ = ref.run_tracker(frames, rows, width, HW, MT, assoc=assoc, dtype=np.float64)
    assert aref.margins_hold(s64), s64.margins
    s32, o32, a32 = ref.run_tracker(frames, rows, width, HW, MT, assoc=assoc)
    rec = torch.from_numpy(_track_ref.pack_records(frames, width)).cuda()
    par = ops.track_params(HW, 'iou')
    tas = ops.track_assoc(**assoc) if assoc else None
    F = len(frames)
    for cuts in ([F], [3, F - 3]):
        out, state = _launch(rec, rows, par, family, tas, cuts, width)
        for f, (w64, w32) in enumerate(zip(o64, o32)):
            assert all(w64[k] == w32[k] for k in ('id', 'missed', 'count', 'dropped'))
            assert out['id'][f].tolist() == w32['id'] and out['missed'][f].tolist() == w32['missed'], (family, f, out['id'][f][:4])
            assert int(out['count'][f]) == w32['count'] and int(out['dropped'][f]) == 0
            if f == BAD_FRAME:
                assert w32['count'] == _track_ref.BAD_CLASS
                continue
            assert out['id'][f, :3].tolist() == [1, 2, 3] and out['missed'][f, :3].tolist() == [0, 0, 0], (family, f)
            assert np.array_equal(_bits(out['box'][f]), _bits(a32[f]['x'].T.copy())), (family, width, f)
            assert np.array_equal(_bits(out['score'][f]), _bits(a32[f]['score'])), (family, f)
        _assert_state_equals(state, [s32], (family, width))
    # the bad-class frame left the state alone: the arrays of the restatement before and after it are the same
    assert all(np.array_equal(_bits(a32[BAD_FRAME][k]), _bits(a32[BAD_FRAME - 1][k])) for k in a32[0])
    plain, _ = _launch(rec, None, par, family, tas, [F], width)
    assert int(plain['id'].max()) > 3


@pytest.mark.parametrize('width', (4, 5))
def test_a_pure_shift_row_gives_the_bits_of_the_shift_entry_point_and_null_those_of_the_old_one(width):
    from mydetection_amd import ops
    frames, shifts = mref.tracker_scenario(width=width, still=4)
    rec = torch.from_numpy(_track_ref.pack_records(frames, width)).cuda()
    par = ops.track_params(mref.TRACK_HW, 'iou')
    rows = np.zeros((len(frames), 8), np.int32)
    rows[:, 2], rows[:, 3], rows[:, 4], rows[:, 6], rows[:, 7] = shifts[:, 0] << 16, shifts[:, 1] << 16, 65536, shifts[:, 2], shifts[:, 3]
    rows[shifts[:, 2] == 0] = 0
    for assoc in (None, ops.track_assoc(**OPTIMAL_BANDS)):
        s1, s2, s3, s4 = (ops.track_state(1, 16, 'cuda') for _ in range(4))
        by_shift = ops.track_frames(rec, s1, par, assoc=assoc, shift=torch.from_numpy(shifts).cuda().view(1, -1, 4))
        by_warp = ops.track_frames(rec, s2, par, assoc=assoc, warp=torch.from_numpy(rows).cuda().view(1, -1, 8))
        assert all(torch.equal(by_shift[k].view(torch.int32) if by_shift[k].dtype == torch.float32 else by_shift[k],
                               by_warp[k].view(torch.int32) if by_warp[k].dtype == torch.float32 else by_warp[k]) for k in by_shift)
        assert torch.equal(s1, s2) and by_shift['id'][0, -1, :3].tolist() == [1, 2, 3]
        # no camera motion at all: the old entry point; rows that are all invalid: the same bits
        old = ops.track_frames(rec, s3, par, assoc=assoc)
        none = ops.track_frames(rec, s4, par, assoc=assoc, warp=torch.zeros((1, len(frames), 8), dtype=torch.int32, device='cuda'))
        assert all(torch.equal(old[k].view(torch.int32) if old[k].dtype == torch.float32 else old[k],
                               none[k].view(torch.int32) if none[k].dtype == torch.float32 else none[k]) for k in old)
        assert torch.equal(s3, s4)
    # the same two equalities through every entry-point family, the appearance ones included
    for family, a in sorted(FAMILIES.items()):
        tas = ops.track_assoc(**a) if a else None
        by_shift, st1 = _launch(rec, None, par, family, tas, [len(frames)], width, shifts=shifts)
        by_warp, st2 = _launch(rec, rows, par, family, tas, [len(frames)], width)
        old, st3 = _launch(rec, None, par, family, tas, [len(frames)], width)
        none, st4 = _launch(rec, np.zeros_like(rows), par, family, tas, [len(frames)], width)
        for k in by_shift:
            assert np.array_equal(_bits(by_shift[k]), _bits(by_warp[k])) and np.array_equal(_bits(old[k]), _bits(none[k])), (family, k)
        assert torch.equal(st1, st2) and torch.equal(st3, st4) and by_warp['id'][-1, :3].tolist() == [1, 2, 3], family
        assert not torch.equal(st1, st3), family
    with pytest.raises(ValueError, match='warp'):
        ops.track_frames(rec, s4, par, warp=torch.zeros((1, 2, 8), dtype=torch.int32, device='cuda'))
    with pytest.raises(ValueError, match='shift and warp'):
        ops.track_frames(rec, s4, par, shift=torch.zeros((1, len(frames), 4), dtype=torch.int32, device='cuda'),
                         warp=torch.zeros((1, len(frames), 8), dtype=torch.int32, device='cuda'))


@pytest.mark.parametrize('family', ('plain', 'appear', 'appear_optimal'))
def test_warp_null_through_the_new_symbols_gives_the_bits_of_the_existing_entry_point(family):
    """ops.track_frames(warp=None) goes to the existing symbols, so the new ones are called here directly with warp = NULL:
    every output and the states equal those of their siblings with shift = NULL."""
    import ctypes
    from mydetection_amd import _lib, ops
    frames, _ = scenario(5)
    rec = torch.from_numpy(_track_ref.pack_records(frames, 5)).cuda()
    F, par = rec.shape[0], ops.track_params(HW, 'iou')
    assoc = ops.track_assoc(**(FAMILIES[family] or {}))
    desc = torch.zeros((F, 512, 128), dtype=torch.uint16, device='cuda')
    aset = ops.appear_set(gate=None, reid=None)
    kw = {}
    if family != 'plain':
        kw['appear'] = (aset, desc, ops.appear_state(1, MT, 'cuda'))
    if family == 'appear_optimal':
        kw.update(appear_weight=0, appear_ws=ops.appear_workspace(1, MT, 'cuda'))
    state = ops.track_state(1, MT, 'cuda')
    want = ops.track_frames(rec, state, par, assoc=assoc, **kw)
    # the same call by hand
    got = {k: torch.full_like(v, -7) for k, v in want.items()}
    state2, astate2, ws2 = ops.track_state(1, MT, 'cuda'), ops.appear_state(1, MT, 'cuda'), ops.appear_workspace(1, MT, 'cuda')
    r3 = rec.view(1, F, -1)
    args = [ops._ptr(r3), r3.stride(0), r3.stride(1), 1, F, 5, ctypes.byref(par), MT, ops._ptr(state2)]
    args += [ops._ptr(got[k]) for k in ('box', 'score', 'cls', 'id', 'missed', 'count', 'dropped')] + [ctypes.byref(assoc), None]
    if family != 'plain':
        args += [ctypes.byref(aset), ops._ptr(desc), ops._ptr(astate2), ops._ptr(got['sim']), ops._ptr(got['how'])]
    if family == 'appear_optimal':
        args += [0, ops._ptr(ws2)]
    name = {'plain': 'mydet_track_frames_warp_f32', 'appear': 'mydet_track_frames_appear_warp_f32',
            'appear_optimal': 'mydet_track_frames_appear_optimal_warp_f32'}[family]
    assert getattr(_lib.lib(), name)(*args, ops._stream()) == 0
    for k in want:
        assert np.array_equal(_bits(got[k].cpu().numpy()), _bits(want[k].cpu().numpy())), (family, k)
    assert torch.equal(state, state2) and int(want['id'].max()) > 3
    if family != 'plain':
        assert torch.equal(kw['appear'][2], astate2)


def test_the_sign_of_the_turn():
    """A positive b (the image turns the x axis towards y) moves a box right of the centre down and raises its angle."""
    from mydetection_amd import ops
    box = np.array([[520.0, 240.0, 20.0, 30.0, 30.0]], np.float32)
    frames = [(box, np.array([0.9], np.float32), np.array([0], np.int64))] * 2
    rec = torch.from_numpy(_track_ref.pack_records(frames, 5)).cuda()
    rows = np.zeros((2, 8), np.int32)
    rows[1] = warp_row(2.0, 1.0, (0.0, 0.0))
    # the second frame holds no detection the track could take: the output is the prediction
    rec[1, 0] = 0
    out = ops.track_frames(rec, ops.track_state(1, 16, 'cuda'), ops.track_params(HW, 'iou'), warp=torch.from_numpy(rows).cuda().view(1, 2, 8))
    x = out['box'][0, 1, 0].cpu().numpy()
    assert abs(x[1] - (240.0 + 200.0 * math.sin(math.radians(2.0)))) < 0.01 and abs(x[0] - (320.0 + 200.0 * math.cos(math.radians(2.0)))) < 0.01
    assert abs(x[4] - 32.0) < 0.002 and int(out['missed'][0, 1, 0]) == 1


# ---- behaviour: this is what the model is for ----

FRAME_HW = (320, 448)
TURN = (3.0, 1.03, (0.0, 0.0))


def _behaviour():
    """Eight boxes of 10 px fixed in the world at radius 100 .. 150 px round the frame centre; three still frames, then one
    turned by 3 degrees and zoomed by 1.03.  Returns (grey frames uint8 [4, H, W], frames for pack_records)."""
    truth = ref.true_model(*TURN)
    grey = ref.scene(FRAME_HW, 1, [truth])
    grey = np.stack([grey[0], grey[0], grey[0], grey[1]])
    ang = np.arange(8) * (2 * math.pi / 8) + 0.2
    rad = np.array([100.0, 150.0, 120.0, 140.0, 110.0, 150.0, 130.0, 105.0])
    cx, cy = FRAME_HW[1] / 2 + rad * np.cos(ang), FRAME_HW[0] / 2 + rad * np.sin(ang)
    still = np.stack([cx, cy, np.full(8, 10.0), np.full(8, 10.0)], axis=1)
    mx, my = ref.apply_model(truth, FRAME_HW, cx, cy)
    turned = np.stack([mx, my, np.full(8, 10.0 * TURN[1]), np.full(8, 10.0 * TURN[1])], axis=1)
    scores, cats = np.full(8, 0.9, np.float32), np.zeros(8, np.int64)
    assert still[:, 0].min() > 10 and still[:, 1].min() > 5 and turned[:, 1].max() < FRAME_HW[0] - 5
    return grey, [(b.astype(np.float32), scores, cats) for b in (still, still, still, turned)]


def test_a_turning_and_zooming_camera_keeps_every_id_only_under_the_similarity_model():
    from mydetection_amd import ops
    grey, frames = _behaviour()
    # on the CPU first: without a model of the turn the restatement loses ids, and so it does with the shift that the shift
    # model's restatement reports for these frames
    _, outs, _ = ref.run_tracker(frames, None, 4, FRAME_HW, 16)
    assert sorted(outs[2]['id'][:8]) == list(range(1, 9)) and max(outs[3]['id']) > 8
    g = mref.Geometry(FRAME_HW, 2, 8)
    cpu_shift, _ = mref.run([mref.Stream(g)], grey.astype(np.int64)[None])
    assert cpu_shift[0, :, 2].tolist() == [0, 1, 1, 1] and np.abs(cpu_shift[0, 3, :2]).max() <= 1
    stream = mref.ShiftStream(16, _track_ref.Params(FRAME_HW, np.float32, match='iou'))
    cpu_ids = [stream.step(*_track_ref.unpack_frame(r, 4), shift=cpu_shift[0, f])['id']
               for f, r in enumerate(_track_ref.pack_records(frames, 4))]
    assert sorted(cpu_ids[2][:8]) == list(range(1, 9)) and max(cpu_ids[3]) > 8
    rgb = torch.from_numpy(np.repeat(grey[..., None], 3, axis=-1)).cuda()
    rec = torch.from_numpy(_track_ref.pack_records(frames, 4)).cuda()
    par = ops.track_params(FRAME_HW, 'iou')
    ids = {}
    for model in ('similarity', 'shift', None):
        state = ops.track_state(1, 16, 'cuda')
        cam = {}
        if model is not None:
            mset = ops.motion_set(model=model, reduce=2, search=8)
            m = ops.motion_frames(rgb, ops.motion_state(1, FRAME_HW, mset, 'cuda'), mset)
            assert m['shift'][0, :, 2].tolist() == [0, 1, 1, 1]
            cam = {'warp': m['warp']} if model == 'similarity' else {'shift': m['shift']}
            if model == 'shift':
                assert np.array_equal(m['shift'].cpu().numpy(), cpu_shift)
            if model == 'similarity':
                row = m['warp'][0, 3].cpu().numpy()
                assert row[6] == 1 and ref.corner_error(row, ref.true_model(*TURN), FRAME_HW) < 0.5
                assert m['warp'][0, 1].tolist() == [0, 0, 0, 0, 65536, 0, 1, 117]
        out = ops.track_frames(rec, state, par, **cam)
        ids[model] = out['id'][0].cpu().numpy()
        assert sorted(ids[model][2][:8].tolist()) == list(range(1, 9))
    assert np.array_equal(ids['similarity'][3], ids['similarity'][2]) and ids['similarity'][3].max() == 8
    for model in ('shift', None):
        assert ids[model][3].max() > 8, model                        # at least one object came back under a new id
    assert [row.tolist() for row in ids['shift']] == cpu_ids         # what the host run said it would be


# ---- the Detector ----

@pytest.fixture(scope='module')
def detector():
    from mydetection_amd import synth
    from mydetection_amd.api import Detector
    from mydetection_amd.models.general import name_to_model
    m, cfg = name_to_model('rapid')
    m.load_state_dict(synth.make_state_dict(m.state_dict(), 'rapid'), strict=True)
    return Detector(model_and_cfg=(m.eval().cuda(), cfg))


def test_frame_methods_with_the_similarity_model(detector):
    """predict_frames(frames, tracker=, motion=CameraMotion(model='similarity')) is ops.motion_frames plus
    ops.track_frames(warp=) on the call's records; with keyframes= the carry reads last['shift']."""
    from mydetection_amd import ops
    from mydetection_amd.api import CameraMotion, KeyFrames, Tracker
    det = detector
    hw = (150, 200)
    truths = [ref.true_model(1.0, 1.01, (2.0, -1.0)), ref.true_model(-1.5, 0.99, (-3.0, 2.0)), ref.true_model(0.5, 1.0, (4.0, 4.0))]
    frames = np.ascontiguousarray(np.stack([ref.scene(hw, seed, truths, margin=32) for seed in (1, 2, 3)], axis=-1))
    kw = dict(input_size=128, conf_thres=0.001)
    tkw = dict(min_score=0.0005, max_tracks=64)
    cam, trk = CameraMotion(model='similarity'), Tracker(**tkw)
    got = det.predict_frames(frames, tracker=trk, motion=cam, **kw)
    assert cam.last['warp'].is_cuda and cam.last['warp'].shape == (1, 4, 8) and cam.last['warp'][0, 1:, 6].tolist() == [1, 1, 1]
    (_, r), = det._frame_records(frames, _whole_records=True, **kw)
    mset = ops.motion_set(model='similarity')
    m = ops.motion_frames(torch.from_numpy(frames).cuda(), ops.motion_state(1, hw, mset, 'cuda'), mset)
    assert torch.equal(m['warp'], cam.last['warp']) and torch.equal(m['shift'], cam.last['shift'])
    state = ops.track_state(1, 64, 'cuda')
    par = ops.track_params(hw, 'rotated', new_thres=kw['conf_thres'], min_score=tkw['min_score'])
    want = ops.track_frames(r, state, par, warp=m['warp'])
    assert torch.equal(state, trk.state)
    keep = (want['missed'].view(4, 64) == 0)
    assert [len(o) for o in got] == keep.sum(dim=1).tolist() and sum(len(o) for o in got) > 0
    for f, o in enumerate(got):
        assert torch.equal(o.obj_ids, want['id'].view(4, 64)[f][keep[f]]) and torch.equal(o.bboxes, want['box'].view(4, 64, 5)[f][keep[f]])
    # the rows did something: the same records with the centre's shift alone leave another state
    state2 = ops.track_state(1, 64, 'cuda')
    ops.track_frames(r, state2, par, shift=m['shift'])
    assert not torch.equal(state, state2)
    # the default model is the object of old: no 'warp', and the call is the shift call
    plain = CameraMotion()
    det.predict_frames(frames, tracker=Tracker(**tkw), motion=plain, **kw)
    assert sorted(plain.last) == ['blocks', 'shift']
    # key frames: the carry takes the centre's shift of the same object
    cam2 = CameraMotion(model='similarity')
    objs = det.predict_frames(frames, tracker=Tracker(**tkw), motion=cam2, keyframes=KeyFrames(every=2), **kw)
    assert len(objs) == 4 and torch.equal(cam2.last['shift'], m['shift']) and torch.equal(cam2.last['warp'], m['warp'])
