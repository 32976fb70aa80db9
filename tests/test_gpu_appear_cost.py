"""GPU tests of the optimal assignment on the fused IoU-and-appearance cost (mydet_track_frames_appear_optimal_f32) against the
restatement tests/_appear_cost_ref.py: == on ids, missed, count, dropped, sim and how, on the tracker state, on `has` and every
template word and on the needed words of the workspace; boxes and scores bit for bit as tests/test_gpu_appear.py checks them.
Every case asserts margins_hold on the restatement before it looks at the kernel (tests/test_appear_cost_host.py proves the
cases on the CPU).  The figures of a failing comparison are in the assertion's message."""
import ctypes

import numpy as np
import pytest
import torch

import _appear_cost_cases as cases
import _appear_cost_ref as ref
import _appear_ref
import _track_ref

pytestmark = pytest.mark.gpu

STATE_KEYS = ('x', 'v', 'pxx', 'pxv', 'pvv', 'score', 'cls', 'id', 'missed')
OUT_KEYS = ('box', 'score', 'cls', 'id', 'missed', 'count', 'dropped')


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def _launch(streams, width, mt, match='iou', appear=None, assoc=None, shifts=None, weight=128, cuts=None, plain=False):
    """streams: [(frames, descs)] of one F.  Through ops.track_frames on fresh states and a workspace of 0x5A bytes, in calls of
    `cuts` frames: per stream (outputs [F, ...], tracker state views, appearance state views, workspace [512, mt]), all numpy.
    plain: the entry point without an appearance (mydet_track_frames_motion_f32) on the same records."""
    from mydetection_amd import ops
    S, F = len(streams), len(streams[0][0])
    rec = _dev(np.concatenate([_track_ref.pack_records(fr, width) for fr, _ in streams])).view(S, F, -1)
    desc = _dev(np.stack([d for _, d in streams]))
    par = ops.track_params(cases.TRACK_HW, match)
    tas = ops.track_assoc('optimal', **(assoc or {}))
    aset = ops.appear_set(**dict(dict(gate=None, reid=None, momentum=0.8, reach=2.0, update_thres=0.5), **(appear or {})))
    state, astate = ops.track_state(S, mt, 'cuda'), ops.appear_state(S, mt, 'cuda')
    ws = ops.appear_workspace(S, mt, 'cuda').fill_(0x5A5A5A5A)
    outs, lo = [], 0
    for n in (cuts or [F]):
        sh = None if shifts is None else _dev(np.stack(shifts)[:, lo:lo + n])
        if plain:
            outs.append(ops.track_frames(rec[:, lo:lo + n], state, par, assoc=tas, shift=sh))
        else:
            outs.append(ops.track_frames(rec[:, lo:lo + n], state, par, assoc=tas, shift=sh, appear=(aset, desc[:, lo:lo + n].contiguous(), astate),
                                         appear_weight=weight, appear_ws=ws))
        lo += n
    torch.cuda.synchronize()
    res = []
    for s in range(S):
        out = {k: torch.cat([o[k] for o in outs], dim=1)[s].cpu().numpy() for k in outs[0]}
        tv = {k: v[s].cpu().numpy() for k, v in ops.track_state_views(state, mt).items()}
        av = {k: v[s].cpu().numpy() for k, v in ops.appear_state_views(astate, mt).items()}
        res.append((out, tv, av, ws[s].view(512, mt).cpu().numpy()))
    return res


def _assert_equals_restatement(got, stream, outs, arrays, what):
    out, tv, av, ws = got
    assert ref.margins_hold(stream), (what, stream.margins)
    for f, (w, a) in enumerate(zip(outs, arrays)):
        for k in ('id', 'missed', 'sim', 'how'):
            assert out[k][f].tolist() == w[k], (what, f, k, out[k][f].tolist(), w[k])
        assert int(out['count'][f]) == w['count'] and int(out['dropped'][f]) == w['dropped'], (what, f)
        if w['count'] >= 0:
            assert np.array_equal(_bits(out['box'][f]), _bits(a['x'].T.copy())), (what, f)
            assert np.array_equal(_bits(out['score'][f]), _bits(a['score'])) and np.array_equal(out['cls'][f], a['cls']), (what, f)
    last = arrays[-1]
    for k in STATE_KEYS:
        assert np.array_equal(_bits(tv[k]), _bits(last[k])), (what, k)
    assert int(tv['next_id']) == stream.next_id
    assert np.array_equal(av['has'], last['has']) and np.array_equal(av['tmpl'], last['tmpl']), what
    if outs[-1]['count'] >= 0:                                        # the workspace contract: the needed pairs of the last frame
        bad = {(d, j): (int(ws[d, j]), s) for (d, j), s in stream.needed.items() if int(ws[d, j]) != s}
        assert not bad, (what, bad)


# ---- 1. the swap ----

@pytest.mark.parametrize('neighbour', (False, True))
def test_the_fused_cost_keeps_the_ids_the_iou_assignment_swaps(neighbour):
    """The test that fails without the feature.  ops level: the optimal assignment alone gives each track the OTHER object; with
    the appearance at weight 128 each keeps its own.  In the second scene the neighbour's colours pass the default gate, so the
    greedy walk with the gate swaps too."""
    from mydetection_amd import ops
    frames, descs, stream, outs, arrays = cases.restated('swap', neighbour, 128)
    appear = dict(gate=0.3, reid=0.6)
    (plain, _, _, _), = _launch([(frames, descs)], 4, 64, plain=True)
    got, = _launch([(frames, descs)], 4, 64, appear=appear, weight=128)
    assert plain['id'][3, :2].tolist() == [1, 2] == got[0]['id'][3, :2].tolist() and (plain['missed'][3, :2] == 0).all()
    # track 1 stood at 200 and its object is now at 212, track 2 at 216 and its object at 204: the filter moves a track most of
    # the way to the detection it took
    assert plain['box'][3, 0, 0] < 204 and plain['box'][3, 1, 0] > 212                               # swapped
    assert got[0]['box'][3, 0, 0] > 206 and got[0]['box'][3, 1, 0] < 210                             # kept
    assert got[0]['sim'][3, :2].tolist() == [131072, 131072] and got[0]['how'][3, :2].tolist() == [1, 1]
    _assert_equals_restatement(got, stream, outs, arrays, ('swap', neighbour))
    if neighbour:
        par, aset = ops.track_params(cases.TRACK_HW), ops.appear_set(gate=0.3, reid=None, momentum=0.8, update_thres=0.5)
        state, astate = ops.track_state(1, 64, 'cuda'), ops.appear_state(1, 64, 'cuda')
        greedy = ops.track_frames(_dev(_track_ref.pack_records(frames, 4)), state, par, appear=(aset, _dev(descs), astate))
        assert greedy['sim'][0, 3, :2].tolist() == [65536, 65536] and float(greedy['box'][0, 3, 0, 0]) < 204             # through the gate, swapped


@pytest.fixture(scope='module')
def detector():
    from mydetection_amd import synth
    from mydetection_amd.api import Detector
    from mydetection_amd.models.general import name_to_model
    m, cfg = name_to_model('rapid')
    m.load_state_dict(synth.make_state_dict(m.state_dict(), 'rapid'), strict=True)
    return Detector(model_and_cfg=(m.eval().cuda(), cfg))


def test_the_swap_through_detector_predict_frames(detector, monkeypatch):
    """Synthetic frames with two painted objects; the call's records are the scene's (the network with synthetic weights finds
    no painted object), everything behind them is the call's own: the descriptor launch on the frames, the routing of
    Appearance(weight=0.5) to the fused entry point, the workspace beside the state."""
    from mydetection_amd import ops
    from mydetection_amd.api import Appearance, Tracker
    frames, recs = cases.painted_swap()
    rec = dict(ops.record_views(_dev(_track_ref.pack_records(recs, 5))), img_hw=[frames.shape[1:3]] * 4)
    monkeypatch.setattr(detector, '_source_records', lambda sources, call: [(list(range(4)), rec)])
    kw = dict(conf_thres=0.3)
    plain = detector.predict_frames(frames, tracker=Tracker(assign='optimal', max_tracks=64), **kw)
    ap = Appearance(weight=0.5)
    fused = detector.predict_frames(frames, tracker=Tracker(assign='optimal', max_tracks=64), appearance=ap, **kw)
    for objs in (plain, fused):
        assert [o.obj_ids.tolist() for o in objs] == [[1, 2]] * 4
    # id 1 stood at x = 100 and its object is now at 118; id 2 at 121 and its object at 103
    assert float(plain[3].bboxes[0, 0]) < 105 and float(plain[3].bboxes[1, 0]) > 116                 # swapped
    assert float(fused[3].bboxes[0, 0]) > 110 and float(fused[3].bboxes[1, 0]) < 111                 # kept
    assert ap.last['sim'][0, 3, :2].tolist() == [131072, 131072] and ap.last['how'][0, 3, :2].tolist() == [1, 1]
    assert ap.workspace.shape == (1, 512 * 64) and ap.workspace.device == ap.state.device
    assert ap.workspace[0].view(512, 64)[:2, :2].tolist() == [[131072, 49152], [49152, 131072]]       # S of the four needed pairs
    # the refusals come before any launch: the trackers stay unbound
    for tracker, appearance, text in ((Tracker(max_tracks=64), Appearance(weight=0.5), "assign='optimal'"),
                                      (Tracker(assign='optimal', max_tracks=64), Appearance(), 'greedy')):
        with pytest.raises(ValueError, match=text):
            detector.predict_frames(frames, tracker=tracker, appearance=appearance, **kw)
        assert tracker.state is None and appearance.state is None


# ---- 2. shapes ----

@pytest.mark.parametrize('mt', sorted(cases.GRID_NS))
def test_shapes_equal_the_restatement(mt):
    """max_tracks 1, 64, 65, 512 against n 0, 1, 2, 63, 64, 65, 512, F = 4: pairs of neighbours the appearance tells apart, a
    template update in every frame, births whose templates decide the next frame's costs -- at 512 in slots >= 64 against
    detections whose S another wave computed."""
    frames, descs, stream, outs, arrays = cases.restated('grid', mt)
    got, = _launch([(frames, descs)], 4, mt, appear=dict(gate=0.3), weight=128)
    _assert_equals_restatement(got, stream, outs, arrays, ('grid', mt))


def test_a_crowd_takes_the_dense_form_of_the_similarity_phase():
    frames, descs, stream, outs, arrays = cases.restated('crowd')
    got, = _launch([(frames, descs)], 4, 128, weight=128)
    _assert_equals_restatement(got, stream, outs, arrays, 'crowd')
    assert len(stream.needed) >= 20


# ---- 3. instances and settings, 4. invariants ----

@pytest.mark.parametrize('key', cases.SETTINGS, ids=lambda k: '-'.join(str(v) for v in k))
def test_instances_and_settings_equal_the_restatement(key):
    """BW 4, BW 5, ROT; bands off and on; shift given and NULL; gate, reid and every weight; a bad-class frame in the middle; in
    one launch and in two (F1 + F2 leaves what F leaves)."""
    variant, bands, shift, gate, reid, weight = key
    v = cases.VARIANTS[variant]
    frames, descs, stream, outs, arrays = cases.restated('settings', *key)
    sh = [cases.shifts_of(len(frames))] if shift else None
    for cuts in (None, [4, 3]):
        got, = _launch([(frames, descs)], v['width'], 64, v['match'], appear=cases.appear_kw(gate, reid)[0], assoc=cases.BANDS if bands else None,
                       shifts=sh, weight=weight, cuts=cuts)
        _assert_equals_restatement(got, stream, outs, arrays, (key, cuts))


@pytest.mark.parametrize('key', [k for k in cases.SETTINGS if k[3:] == (0.0, 0.0, 0)], ids=lambda k: '-'.join(str(v) for v in k))
def test_weight_gate_and_reid_off_is_the_plain_optimal_launch(key):
    """weight == 0, gate == 0, reid == 0: every output and every word of the tracker state of mydet_track_frames_motion_f32 with
    the same optimal assoc, bit for bit."""
    variant, bands, shift, _, _, _ = key
    v = cases.VARIANTS[variant]
    frames, descs, stream, outs, arrays = cases.restated('settings', *key)
    for sh in (None, [cases.shifts_of(len(frames))]):
        kw = dict(assoc=cases.BANDS if bands else None, shifts=sh)
        (new, tv, av, _), = _launch([(frames, descs)], v['width'], 64, v['match'], weight=0, **kw)
        (old, tv0, _, _), = _launch([(frames, descs)], v['width'], 64, v['match'], plain=True, **kw)
        assert set(new) == set(old) | {'sim', 'how'}
        for k in old:
            assert np.array_equal(_bits(new[k]), _bits(old[k])), (key, k)
        for k in tv0:
            assert np.array_equal(_bits(tv[k]), _bits(tv0[k])), (key, k)
        assert av['has'].sum() > 0 and int(new['id'].max()) > 6


def test_two_streams_with_different_contents():
    key = ('bw4', True, True, 0.3, 0.5, 128)
    frames, descs, stream, outs, arrays = cases.restated('settings', *key)
    F = len(frames)
    sw_frames, sw_descs = cases.swap(4, True)
    sw_frames = sw_frames + [cases._fr([], 4)] * (F - len(sw_frames))
    sw_descs = np.concatenate([sw_descs, np.zeros((F - len(sw_descs), 512, 128), np.uint16)])
    a, r = cases.appear_kw(0.3, 0.5)
    still = np.zeros((F, 4), np.int32)
    second = ref.run(sw_frames, sw_descs, 4, cases.TRACK_HW, 64, appear=r, assoc=cases.BANDS, shifts=still, weight=128)
    got = _launch([(frames, descs), (sw_frames, sw_descs)], 4, 64, appear=a, assoc=cases.BANDS, shifts=[cases.shifts_of(F), still], weight=128)
    _assert_equals_restatement(got[0], stream, outs, arrays, 'stream 0')
    _assert_equals_restatement(got[1], *second, 'stream 1')
    assert second[1][3]['match'][:2] == [1, 0]


def test_a_track_without_a_template_keeps_its_iou():
    """has == 0: a track born by the plain optimal launch; m = q whatever the weight, the gate lets it through, and the first
    match gives it a template."""
    from mydetection_amd import ops
    frames, descs, _, _, _ = cases.restated('settings', 'bw4', False, False, 0.3, 0.5, 128)
    frames, descs = frames[:3], descs[:3]
    a, r = cases.appear_kw(0.9, 0.5)
    stream, outs, arrays = ref.run(frames[:1], descs[:1], 4, cases.TRACK_HW, 64, appear=r, weight=256)
    stream.has[:], stream.tmpl[:] = 0, 0                              # the plain launch knows no appearance
    _, more, more_arrays = ref.run(frames[1:], descs[1:], 4, cases.TRACK_HW, 64, weight=256, stream=stream)
    assert ref.margins_hold(stream) and more[0]['how'][:7] == [1] * 7 and more[0]['sim'][:7] == [0] * 7 and more[1]['how'][:7] == [1, 1, 1, 0, 1, 1, 1] and min(v for v in more[1]['sim'][:7] if v >= 0) > 100000
    rec = _dev(_track_ref.pack_records(frames, 4)).view(1, 3, -1)
    par, tas, aset = ops.track_params(cases.TRACK_HW), ops.track_assoc('optimal'), ops.appear_set(**a)
    state, astate, ws = ops.track_state(1, 64, 'cuda'), ops.appear_state(1, 64, 'cuda'), ops.appear_workspace(1, 64, 'cuda')
    ops.track_frames(rec[:, :1], state, par, assoc=tas)
    out = ops.track_frames(rec[:, 1:], state, par, assoc=tas, appear=(aset, _dev(descs[1:]), astate), appear_weight=256, appear_ws=ws)
    for f in range(2):
        for k in ('id', 'missed', 'sim', 'how'):
            assert out[k][0, f].tolist() == more[f][k], (f, k)
    av = ops.appear_state_views(astate, 64)
    assert np.array_equal(av['has'][0].cpu().numpy(), more_arrays[-1]['has']) and np.array_equal(av['tmpl'][0].cpu().numpy(), more_arrays[-1]['tmpl'])


# ---- 5. refusals ----

def test_refusals_launch_nothing_and_touch_no_buffer():
    from mydetection_amd import _lib, ops
    frames, descs = cases.swap()
    rec, d = _dev(_track_ref.pack_records(frames, 4)), _dev(descs)
    state, astate = ops.track_state(1, 64, 'cuda'), ops.appear_state(1, 64, 'cuda')
    ws = ops.appear_workspace(1, 64, 'cuda').fill_(7)
    par = ops.track_params(cases.TRACK_HW)
    F = len(frames)
    outs = {k: torch.full(shape, 7, dtype=dt, device='cuda') for k, (shape, dt) in
            dict(box=((1, F, 64, 5), torch.float32), score=((1, F, 64), torch.float32), cls=((1, F, 64), torch.int64), id=((1, F, 64), torch.int64),
                 missed=((1, F, 64), torch.int32), count=((1, F), torch.int32), dropped=((1, F), torch.int32), sim=((1, F, 64), torch.int32),
                 how=((1, F, 64), torch.int32)).items()}
    s0, a0 = state.clone(), astate.clone()

    def call(assoc, aset=None, weight=128, wsp=None, mt=64):
        aset = ops.appear_set() if aset is None else aset
        return _lib.lib().mydet_track_frames_appear_optimal_f32(
            rec.data_ptr(), rec.stride(0) * F, rec.stride(0), 1, F, 4, ctypes.byref(par), mt, state.data_ptr(),
            *(outs[k].data_ptr() for k in OUT_KEYS), ctypes.byref(assoc), None, ctypes.byref(aset), d.data_ptr(), astate.data_ptr(),
            outs['sim'].data_ptr(), outs['how'].data_ptr(), weight, ws.data_ptr() if wsp is None else wsp, None)
    opt = ops.track_assoc('optimal')
    assert call(ops.track_assoc('greedy')) == -2 and call(ops.track_assoc('greedy', 0.2, 0.5, 0.3)) == -2
    assert call(opt, weight=-1) == -1 and call(opt, weight=257) == -1
    assert call(opt, wsp=ctypes.c_void_p(None)) == -1 and call(opt, wsp=ws.data_ptr() + 4) == -1
    bad = ops.appear_set()
    bad.alpha = 0
    assert call(opt, aset=bad) == -1 and call(opt, mt=513) == -2 and call(opt, mt=0) == -1
    torch.cuda.synchronize()
    assert torch.equal(state, s0) and torch.equal(astate, a0) and bool((ws == 7).all()) and all(bool((t == 7).all()) for t in outs.values())
    ap = (ops.appear_set(), d, astate)
    with pytest.raises(ValueError, match="assign 'optimal' only"):
        ops.track_frames(rec, state, par, appear=ap, appear_weight=128, appear_ws=ws)
    with pytest.raises(ValueError, match='greedy'):
        ops.track_frames(rec, state, par, assoc=opt, appear=ap)
    with pytest.raises(ValueError, match='appear_ws'):
        ops.track_frames(rec, state, par, assoc=opt, appear=ap, appear_weight=128, appear_ws=ws[:, :-4].contiguous())
    with pytest.raises(ValueError, match='appear_ws'):
        ops.track_frames(rec, state, par, assoc=opt, appear=ap, appear_weight=128, appear_ws=ws.cpu())
    torch.cuda.synchronize()
    assert torch.equal(state, s0) and torch.equal(astate, a0) and bool((ws == 7).all())
    assert call(opt) == 0                                             # and the same buffers run
    torch.cuda.synchronize()
    assert outs['id'][0, 3, :2].tolist() == [1, 2] and not torch.equal(state, s0)
