"""CPU tests of tracking across video frames: the numpy restatement tests/_track_ref.py against the reference's KFTracklet
(tests/golden/kf_tracklet.npz, written by tools/gen_golden_track.py) in float64 and float32, the association rules on the
hand-made cases of tests/_track_cases.py, the C ABI (declared, exported, bound, constants, argument checks before any launch)
and the argument errors of api.Tracker, ops.track_frames and Detector(..., tracker=) on a meta-device model."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import _track_cases as tc
import _track_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {'mydet_track_state_words': 1, 'mydet_track_reset': 4, 'mydet_track_frames_f32': 17}
BLOCKS = (('pxx', 0, 0), ('pxv', 0, 5), ('pxv', 5, 0), ('pvv', 5, 5))


def _run_fixture(g, dtype):
    """Every sequence of the fixture through ref.Track: per sequence a list of (track snapshot, step index)."""
    par = ref.Params(tuple(g['img_hw']), dtype)
    out = []
    for i in range(len(g['names'])):
        t = ref.Track(g['init_box'][i], g['init_score'][i], 0, 1, par)
        steps = []
        for k in range(int(g['length'][i])):
            t.predict(par)
            if g['has_z'][i, k]:
                t.update(g['z'][i, k], g['z_score'][i, k], par)
            steps.append({'x': np.concatenate([t.x, t.v]), 'pxx': t.pxx, 'pxv': t.pxv, 'pvv': t.pvv, 'score': t.score,
                          'missed': t.missed, 'feasible': t.feasible(par), 'box': t.box})
        out.append(steps)
    return out


def test_fixture_covers_the_sequences_the_filter_can_go_wrong_on(golden):
    g = golden('kf_tracklet')
    names = list(g['names'])
    assert names == ['plain', 'wrap_up', 'wrap_down', 'missed', 'leaving', 'raw_m30', 'raw_400']
    n = {k: int(g['length'][i]) for i, k in enumerate(names)}
    ang = {k: g['x'][i, :n[k], 4] for i, k in enumerate(names)}
    assert (ang['wrap_up'][:4] > 170).all() and (ang['wrap_up'][-4:] < 40).all()            # 179 -> 1
    assert (ang['wrap_down'][:4] < 10).all() and (ang['wrap_down'][-4:] > 140).all()        # 1 -> 179
    assert all(((a >= 0) & (a < 180)).all() for a in ang.values())
    i = names.index('missed')
    assert g['score'][i, n['missed'] - 1] < 0.1 < g['score'][i, 20] and not g['feasible'][i, n['missed'] - 1]
    assert g['pred_count'][i].max() >= 12 and g['pred_count'][i, 9] == 3 and g['pred_count'][i, 10] == 0
    i = names.index('leaving')
    assert g['feasible'][i, 0] and not g['feasible'][i, n['leaving'] - 1] and g['x'][i, n['leaving'] - 1, 0] > 640
    assert g['init_box'][names.index('raw_m30'), 4] == -30 and g['init_box'][names.index('raw_400'), 4] == 400
    assert abs(g['z'][names.index('raw_400'), 0, 4] - 400) < 1.5 and abs(g['z'][names.index('raw_m30'), 0, 4] + 30) < 1.5
    assert max(n.values()) == 40 and g['P'].shape[2:] == (10, 10)


def test_float64_restatement_reproduces_the_reference(golden):
    """Every array of the fixture to 1e-9 relative (the algebra is the reference's up to the order of sums), and the
    covariance entries outside the five 2 x 2 blocks are exactly 0 in the reference itself."""
    g = golden('kf_tracklet')
    off = np.ones((10, 10), bool)
    idx = np.arange(5)
    for a, b in ((idx, idx), (idx, idx + 5), (idx + 5, idx), (idx + 5, idx + 5)):
        off[a, b] = False
    assert off.sum() == 80 and not g['P'][:, :, off].any()
    for i, steps in enumerate(_run_fixture(g, np.float64)):
        for k, s in enumerate(steps):
            what = f"{g['names'][i]} step {k}"
            np.testing.assert_allclose(s['x'], g['x'][i, k], rtol=1e-9, atol=1e-12, err_msg=what)
            for name, r0, c0 in BLOCKS:
                np.testing.assert_allclose(s[name], g['P'][i, k][idx + r0, idx + c0], rtol=1e-9, atol=0, err_msg=what)
            np.testing.assert_allclose(s['score'], g['score'][i, k], rtol=1e-9, err_msg=what)
            np.testing.assert_allclose(s['box'], g['box'][i, k], rtol=1e-9, atol=1e-12, err_msg=what)
            assert s['missed'] == g['pred_count'][i, k] and s['feasible'] == g['feasible'][i, k], what


def test_float32_restatement_stays_within_its_measured_bound(golden):
    """The kernel's operation order in float32 against the float64 reference, over every step of the fixture (up to 40
    predict / update steps, coordinates up to 728 px, so 1 ulp of the largest coordinate is 2^-14 = 6.1e-5 px).
    Measured on the fixture: state (x and v) 1.21e-4 px = 1.98 ulp (sequence 'missed', after 19 predictions without an update);
    covariance blocks 6.3e-7 relative = 5.3 eps; score 1.21e-7 = 2.03 ulp of a score in [0.5, 1).
    Bounds: 4 ulp = 2.44e-4 px (2.0 x the measured maximum), 12 eps = 1.43e-6 relative (2.3 x), 4 ulp = 2.38e-7 (2.0 x).
    The decisions (prediction counter, feasibility) are the reference's exactly."""
    g = golden('kf_tracklet')
    largest = max(np.abs(g['x'][i, :int(g['length'][i]), :4]).max() for i in range(len(g['names'])))
    ulp = float(np.spacing(np.float32(largest)))
    assert ulp == 2.0 ** -14
    idx = np.arange(5)
    worst = {'state': 0.0, 'cov': 0.0, 'score': 0.0}
    for i, steps in enumerate(_run_fixture(g, np.float32)):
        for k, s in enumerate(steps):
            assert s['x'].dtype == np.float32 and s['pxx'].dtype == np.float32 and type(s['score']) is np.float32
            worst['state'] = max(worst['state'], np.abs(s['x'].astype(np.float64) - g['x'][i, k]).max())
            for name, r0, c0 in BLOCKS:
                r = g['P'][i, k][idx + r0, idx + c0]
                worst['cov'] = max(worst['cov'], (np.abs(s[name].astype(np.float64) - r) / np.abs(r)).max())
            worst['score'] = max(worst['score'], abs(float(s['score']) - g['score'][i, k]))
            assert s['missed'] == g['pred_count'][i, k] and s['feasible'] == g['feasible'][i, k], (g['names'][i], k)
    print('float32 restatement, worst over the fixture:', worst, 'ulp of the largest coordinate', ulp)
    assert worst['state'] <= 4 * ulp, worst
    assert worst['cov'] <= 12 * 2.0 ** -23, worst
    assert worst['score'] <= 4 * 2.0 ** -24, worst


def _run_case(case, dtype):
    par = ref.Params(tc.IMG_HW, dtype, match=case['match'], **case['params'])
    stream = ref.Stream(case['max_tracks'], par)
    rec = ref.pack_records(case['frames'], case['width'])
    return stream, [stream.step(*ref.unpack_frame(r, case['width'])) for r in rec]


@pytest.mark.parametrize('name', list(tc.cases()))
def test_association_rules_on_hand_made_cases(name):
    case = tc.cases()[name]
    for dtype in (np.float64, np.float32):
        stream, outs = _run_case(case, dtype)
        assert len(outs) == len(case['expect'])
        for f, (got, want) in enumerate(zip(outs, case['expect'])):
            for key in ('id', 'missed', 'count', 'dropped'):
                assert got[key] == want[key], (name, dtype.__name__, f, key, got[key], want[key])
            assert got['match'] == case['pairs'][f], (name, dtype.__name__, f, got['match'])
        assert stream.ties == case['ties']
        assert stream.margins['iou_thres'] >= 0.05 and stream.margins['iou_gap'] >= 0.05 and stream.margins['score'] >= 1e-3, stream.margins
    if name == 'angle_wrap':
        stream, _ = _run_case(case, np.float64)
        a = stream.slots[0].x[4]
        assert 0 <= a < 180 and min(a, 180 - a) < 2.0
    if name == 'bad_class_frame':
        stream, _ = _run_case(case, np.float64)
        assert stream.slots[0].missed == 0 and stream.next_id == 2


def test_full_size_case_on_the_checker():
    case = tc.full_case()
    stream, outs = _run_case(case, np.float64)
    for got, want in zip(outs, case['expect']):
        assert all(got[k] == want[k] for k in ('id', 'missed', 'count', 'dropped'))
    assert stream.margins['iou_thres'] >= 0.05 and stream.margins['score'] >= 1e-3 and stream.ties == 0
    assert sorted(outs[1]['match']) == list(range(512)) and outs[1]['match'] != outs[0]['match']


def test_record_packing_round_trip():
    from mydetection_amd import _lib
    b = np.arange(15, dtype=np.float32).reshape(3, 5)
    rec = ref.pack_records([(b, [0.5, 0.25, 0.125], [7, 8, 9]), None, (np.zeros((0, 5)), [], [])], 5)
    assert rec.shape == (3, _lib.REC_ROT_WORDS) and rec[:, 0].tolist() == [3, -1, 0]
    ub, us, uc, n = ref.unpack_frame(rec[0], 5)
    assert n == 3 and (ub[:3] == b).all() and us[:3].tolist() == [0.5, 0.25, 0.125] and uc[:3].tolist() == [7, 8, 9]
    assert ref.pack_records([(b[:, :4], [1, 1, 1], [0, 0, 0])], 4).shape == (1, _lib.REC_WORDS)
    v = torch.from_numpy(rec)
    from mydetection_amd import ops
    views = ops.record_views(v)
    assert views['angle'][0, :3].tolist() == [4.0, 9.0, 14.0] and views['bbox'][0, 1].tolist() == [5.0, 6.0, 7.0, 8.0]


def test_entry_points_are_declared_exported_and_bound():
    from mydetection_amd import _lib, ops
    header = open(os.path.join(ROOT, 'include', 'mydet.h')).read()
    assert re.search(r'\bint64_t\s+mydet_track_state_words\s*\(', header)
    assert re.search(r'\bint\s+mydet_track_reset\s*\(', header) and re.search(r'\bint\s+mydet_track_frames_f32\s*\(', header)
    handle = ctypes.CDLL(_lib.LIB_PATH)
    lib = _lib.lib()
    for name, nargs in NAMES.items():
        assert hasattr(handle, name), name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name]) == nargs
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name]
    assert lib.mydet_track_state_words.restype == ctypes.c_int64

    def define(name):
        return int(re.search(r'#define ' + name + r'\s+(-?\d+)', header).group(1))
    assert define('MYDET_TRACK_MAX_TRACKS') == _lib.TRACK_MAX_TRACKS == 512
    assert (define('MYDET_TRACK_STATE_HEADER'), define('MYDET_TRACK_SLOT_WORDS')) == (_lib.TRACK_STATE_HEADER, _lib.TRACK_SLOT_WORDS) == (8, 31)
    assert (define('MYDET_TRACK_MATCH_IOU'), define('MYDET_TRACK_MATCH_ROTATED')) == (_lib.TRACK_MATCH_IOU, _lib.TRACK_MATCH_ROTATED) == (0, 1)
    assert define('MYDET_ABI_VERSION') == _lib.ABI_VERSION == lib.mydet_abi_version() == 2          # new symbols only
    for mt in (1, 3, 4, 256, 512):
        assert lib.mydet_track_state_words(mt) == ops.track_state_words(mt) == (8 + 31 * mt + 3) // 4 * 4
    assert lib.mydet_track_state_words(0) == lib.mydet_track_state_words(513) == 0
    assert ctypes.sizeof(_lib.TrackParams) == 4 * (25 + 6 + 2)
    assert (ref.P0, ref.Q, ref.R) == (ops.TRACK_P0, ops.TRACK_Q, ops.TRACK_R)


def test_state_views_follow_the_documented_layout():
    from mydetection_amd import ops
    mt = 3
    words = ops.track_state_words(mt)
    state = torch.arange(2 * words, dtype=torch.int32).view(2, words)
    v = ops.track_state_views(state)
    row = state[1]
    assert v['next_id'].shape == (2,) and v['live'][1] == row[2]
    assert v['cls'].shape == v['id'].shape == (2, mt) and v['cls'].dtype == v['id'].dtype == torch.int64
    assert v['cls'][1].view(torch.int32).tolist() == row[8:8 + 2 * mt].tolist()
    assert v['id'][1].view(torch.int32).tolist() == row[8 + 2 * mt:8 + 4 * mt].tolist()
    o = 8 + 4 * mt
    for name in ('x', 'v', 'pxx', 'pxv', 'pvv'):
        assert v[name].shape == (2, 5, mt) and v[name].dtype == torch.float32
        assert v[name][1].reshape(-1).view(torch.int32).tolist() == row[o:o + 5 * mt].tolist()
        o += 5 * mt
    assert v['score'][1].view(torch.int32).tolist() == row[o:o + mt].tolist()
    assert v['missed'][1].tolist() == row[o + mt:o + 2 * mt].tolist() and o + 2 * mt <= words < o + 2 * mt + 4
    v['x'][0, 4, 2] = 5.0                                                        # views, not copies
    assert state[0, 8 + 4 * mt + 4 * mt + 2].view(torch.float32) == 5.0
    with pytest.raises(ValueError, match='words'):
        ops.track_state_views(torch.zeros((1, words + 4), dtype=torch.int32), mt)


def test_abi_argument_checks():
    """Every call below must fail before any launch: the pointers are host addresses."""
    from mydetection_amd import _lib, ops
    lib = _lib.lib()
    buf = (ctypes.c_int32 * 64)()
    p = (ctypes.cast(buf, ctypes.c_void_p).value + 15) // 16 * 16
    W4, W5 = _lib.REC_WORDS, _lib.REC_ROT_WORDS
    par = ops.track_params((480, 640))
    rot = ops.track_params((480, 640), match='rotated')

    def call(rec=p, ss=None, fs=None, S=2, F=3, bw=4, params=par, mt=4, state=p, box=p, score=p, cls=p, ids=p, missed=p, count=p,
             dropped=p):
        words = W5 if bw == 5 else W4
        ss = F * words if ss is None else ss
        fs = words if fs is None else fs
        pp = ctypes.byref(params) if params is not None else None
        return lib.mydet_track_frames_f32(rec, ss, fs, S, F, bw, pp, mt, state, box, score, cls, ids, missed, count, dropped, None)
    bad, unsupp = -1, -2
    assert call(S=0) == bad and call(F=0) == bad and call(mt=0) == bad and call(S=-1) == bad
    assert call(bw=3) == bad and call(bw=6) == bad
    assert call(mt=513) == unsupp and call(mt=100000) == unsupp
    assert call(params=rot) == bad                                                # the rotated test needs the angle plane
    wrong = ops.track_params((480, 640))
    wrong.match = 2
    assert call(params=wrong) == bad
    for k in ('rec', 'params', 'state', 'box', 'score', 'cls', 'ids', 'missed', 'count', 'dropped'):
        assert call(**{k: None}) == bad, k
    assert call(rec=p + 4) == bad and call(state=p + 8) == bad and call(cls=p + 4) == bad and call(ids=p + 4) == bad
    assert call(box=p + 2) == bad and call(count=p + 1) == bad
    assert call(ss=3 * W4 + 2) == bad and call(fs=W4 + 1) == bad and call(ss=-3 * W4) == bad and call(fs=-W4) == bad
    assert lib.mydet_track_reset(None, 1, 4, None) == bad and lib.mydet_track_reset(p, 0, 4, None) == bad
    assert lib.mydet_track_reset(p, 1, 0, None) == bad and lib.mydet_track_reset(p + 4, 1, 4, None) == bad
    assert lib.mydet_track_reset(p, 1, 513, None) == unsupp


def test_tracker_value_class():
    from mydetection_amd import ops
    from mydetection_amd.api import Tracker
    t = Tracker()
    assert (t.streams, t.max_tracks, t.match, t.match_thres, t.new_thres, t.max_missed, t.momentum, t.min_score) == \
        (1, 256, None, 0.3, None, 30, 0.8, 0.1)
    assert t.state is None and t.img_hw is None and (t.p0, t.q, t.r) == (ops.TRACK_P0, ops.TRACK_Q, ops.TRACK_R)
    t.reset()                                                                     # nothing bound yet: a no-op
    p = t.params((480, 640), 'rotated', 0.25)
    assert p.new_thres == np.float32(0.25) and p.match == 1 and (p.img_h, p.img_w, p.max_missed) == (480.0, 640.0, 30)
    assert list(p.q) == [float(np.float32(np.float64(v) ** 2)) for v in ops.TRACK_Q] and p.momentum == np.float32(0.8)
    assert Tracker(new_thres=0.5).params((4, 4), 'iou', 0.25).new_thres == 0.5
    assert t.resolve_match('cxcywhd') == 'rotated' and t.resolve_match('cxcywh') == 'iou'
    assert Tracker(match='iou').resolve_match('cxcywhd') == 'iou'
    with pytest.raises(ValueError, match='rotated'):
        Tracker(match='rotated').resolve_match('cxcywh')
    for kw, word in ((dict(streams=0), 'streams'), (dict(max_tracks=0), 'max_tracks'), (dict(max_tracks=513), 'max_tracks'),
                     (dict(match='giou'), 'match'), (dict(max_missed=0), 'max_missed'), (dict(momentum=1.5), 'momentum'),
                     (dict(q=(1, 2, 3)), 'q'), (dict(r=(1, 2, 3, 4, -1)), 'r'), (dict(p0=[float('nan')] * 10), 'p0')):
        with pytest.raises(ValueError, match=word):
            Tracker(**kw)
    with pytest.raises(ValueError, match='multiple'):
        Tracker(streams=2).check_call(3, (480, 640), 'cxcywh')
    t.img_hw, t.box_width = (480, 640), 4
    t.check_call(2, (480, 640), 'cxcywh')
    with pytest.raises(ValueError, match='one frame size'):
        t.check_call(2, (240, 320), 'cxcywh')
    with pytest.raises(ValueError, match='one frame size'):
        t.check_call(2, (480, 640), 'cxcywhd')


def test_track_frames_argument_errors_and_no_cpu_path():
    from mydetection_amd import _lib, ops
    par = ops.track_params((480, 640))
    state = torch.zeros((2, ops.track_state_words(4)), dtype=torch.int32)
    rec = torch.zeros((6, _lib.REC_WORDS), dtype=torch.int32)
    with pytest.raises(RuntimeError, match='no CPU path'):
        ops.track_frames(rec, state, par)
    with pytest.raises(RuntimeError, match='no CPU path'):
        ops.track_reset_(state, 4)
    with pytest.raises(TypeError, match='TrackParams'):
        ops.track_frames(rec, state, {'match': 'iou'})
    with pytest.raises(ValueError, match='records of'):
        ops.track_frames(rec[:, :100], state, par)
    with pytest.raises(ValueError, match='records of'):
        ops.track_frames(rec.float(), state, par)
    with pytest.raises(ValueError, match='streams'):
        ops.track_frames(rec[:5], state, par)
    with pytest.raises(ValueError, match='streams'):
        ops.track_frames(rec, state, par, frames_per_stream=2)
    with pytest.raises(ValueError, match='rotated'):
        ops.track_frames(rec, state, ops.track_params((480, 640), match='rotated'))
    with pytest.raises(ValueError, match='state'):
        ops.track_frames(rec, state[:, :-4].contiguous(), par, max_tracks=4)
    with pytest.raises(ValueError, match='state'):
        ops.track_frames(rec, state.long(), par, max_tracks=4)
    with pytest.raises(ValueError, match='copies'):
        views = ops.record_views(rec)
        ops.track_frames(dict(views, bbox=views['bbox'].clone()), state, par)
    for kw, word in ((dict(match='giou'), 'match'), (dict(max_missed=0), 'max_missed'), (dict(img_hw=(0, 640)), 'frame size'),
                     (dict(q=(1, 2)), 'q')):
        with pytest.raises(ValueError, match=word):
            ops.track_params(**dict(dict(img_hw=(480, 640)), **kw))
    for mt in (0, 513):
        with pytest.raises(ValueError, match='max_tracks'):
            ops.track_state_words(mt)


def _meta_detector(name='yolov3_80'):
    from mydetection_amd.api import Detector
    from mydetection_amd.models.general import name_to_model
    with torch.device('meta'):
        m, cfg = name_to_model(name)
    return Detector(model_and_cfg=(m.eval(), cfg))


def test_detector_rejects_bad_tracked_calls_before_any_gpu_work():
    from mydetection_amd.api import Tracker
    det = _meta_detector()
    assert next(det.model.parameters()).device.type == 'meta'
    a, b = np.zeros((2, 96, 128, 3), np.uint8), np.zeros((1, 128, 96, 3), np.uint8)
    for wrong in ('tracker', True, 4):
        with pytest.raises(TypeError, match='Tracker'):
            det.predict_frames(a, tracker=wrong)
    with pytest.raises(ValueError, match='one size'):
        det.predict_frames([a, b], tracker=Tracker())
    with pytest.raises(ValueError, match='multiple'):
        det.predict_frames(np.zeros((3, 96, 128, 3), np.uint8), tracker=Tracker(streams=2))
    with pytest.raises(ValueError, match='rotated'):                               # yolov3_80 predicts cxcywh
        det.predict_frames(a, tracker=Tracker(match='rotated'))
    bound = Tracker()
    bound.img_hw, bound.box_width = (48, 64), 4
    with pytest.raises(ValueError, match='one frame size'):
        det.predict_frames(a, tracker=bound)
    with pytest.raises(TypeError, match='float32'):                                # the frame rules hold as without a tracker
        det.predict_frames(np.zeros((2, 8, 8, 3), np.float32), tracker=Tracker())
    y, uv = np.zeros((3, 96, 128), np.uint8), np.zeros((3, 48, 64, 2), np.uint8)
    with pytest.raises(ValueError, match='multiple'):
        det.predict_frames_yuv((y, uv), 'nv12', tracker=Tracker(streams=2))
    with pytest.raises(ValueError, match='multiple'):
        det.predict_frames_nv12(y, uv, tracker=Tracker(streams=2))
    with pytest.raises(TypeError, match='Tracker'):
        det.predict_frames_nv12(y, uv, tracker=object())
    with pytest.raises(TypeError, match='json'):
        det.frames_to_json(a, [0, 1], tracker=Tracker())
    with pytest.raises(TypeError, match='json'):
        det.frames_nv12_to_json(y, uv, [0, 1, 2], tracker=Tracker())


def test_image_objects_carry_obj_ids():
    from mydetection_amd.utils.structures import ImageObjects
    boxes, cats, scores = torch.rand(3, 4), torch.tensor([1, 2, 1]), torch.tensor([0.2, 0.9, 0.5])
    assert ImageObjects(boxes, cats, None, scores).obj_ids is None
    o = ImageObjects(boxes, cats, None, scores, obj_ids=torch.tensor([7, 8, 9]))
    assert o[1].obj_ids.tolist() == [8] and o[0:2].obj_ids.tolist() == [7, 8] and ImageObjects(boxes, cats, None, scores)[1].obj_ids is None
    o.sort_by_score_()
    assert o.obj_ids.tolist() == [8, 9, 7]
    o.category_filter_([1])
    assert o.obj_ids.tolist() == [9, 7] and o.cats.tolist() == [1, 1]
