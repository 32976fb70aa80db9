"""GPU tests of the tracker's association modes (include/mydet.h: mydet_track_assoc, mydet_track_frames_assoc_f32; csrc/track.hip,
csrc/hung.h): the optimal assignment and the low-score second stage.

The checker is tests/_assoc_ref.py.  Every case asserts its margins on the float64 restatement first (>= 0.05 for an IoU to its
stage's threshold, >= 1e-3 for a score, >= 0.05 * 65536 between the optimal total and the total of any other pairing), so the
kernel's float32 IoUs decide alike; the kernel is then held to the expected id, missed, count and dropped of every slot and
frame, and its state planes to the float32 restatement bit for bit.  Synthetic records with integer-valued boxes in a 480 x 640
frame everywhere; only the end-to-end test runs a model.  Every launch is synchronised before it is compared."""
import ctypes

import numpy as np
import pytest
import torch

import _assoc_cases as ac
import _assoc_ref as aref
import _mot_ref
import _track_cases as tc
import _track_ref as ref
from test_gpu_track import _assert_state_equals, _bits, _synthetic_frames

pytestmark = pytest.mark.gpu

OUT_KEYS = ('box', 'score', 'cls', 'id', 'missed', 'count', 'dropped')
E2E_CONF = 0.3                                       # the synthetic weights score up to 0.8, about ten detections per frame above 0.3


def _track(rec, state, par, assoc):
    from mydetection_amd import ops
    out = ops.track_frames(torch.from_numpy(rec).cuda() if isinstance(rec, np.ndarray) else rec, state, par, assoc=assoc)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _check_case(case, what, streams=1, launches=1):
    """`case` on the float64 restatement (margins, expectations), then on the kernel: every frame in `launches` launches.  With
    streams > 1, case['frames'] is a list of per-stream frame lists of one length."""
    from mydetection_amd import ops
    hw, mt, width = ac.IMG_HW, case['max_tracks'], case['width']
    per_stream = case['frames'] if streams > 1 else [case['frames']]
    F = len(per_stream[0])
    want, f32s, boxes, scores = [], [], [], []
    for s, frames in enumerate(per_stream):
        one = dict(case, frames=frames)
        chk, w = aref.run_case(one, np.float64, hw)
        assert aref.margins_hold(chk), (what, s, chk.margins, chk.unchecked)
        assert chk.ties == case['ties'], (what, s, chk.ties)
        if case.get('expect') is not None:
            for got, e in zip(w, case['expect']):
                assert all(got[k] == e[k] for k in ('id', 'missed', 'count', 'dropped')), (what, got, e)
        par32 = ref.Params(hw, np.float32, match=case['match'], **case['params'])
        f32 = aref.Stream(mt, par32, **case['assoc'])
        bx, sc = [], []
        for r, w64 in zip(ref.pack_records(frames, width), w):
            got32 = f32.step(*ref.unpack_frame(r, width))
            assert all(got32[k] == w64[k] for k in ('id', 'missed', 'count', 'dropped', 'match')), (what, s)
            a = f32.arrays()
            bx.append(a['x'].T.copy())
            sc.append(a['score'].copy())
        want.append(w)
        f32s.append(f32)
        boxes.append(bx)
        scores.append(sc)
    rec = np.stack([ref.pack_records(frames, width) for frames in per_stream])          # [S, F, words]
    par = ops.track_params(hw, case['match'], **case['params'])
    assoc = ops.track_assoc(**case['assoc'])
    state = ops.track_state(streams, mt, 'cuda')
    step = F // launches
    outs = [_track(np.ascontiguousarray(rec[:, f0:f0 + step]), state, par, assoc) for f0 in range(0, F, step)]
    out = {k: np.concatenate([o[k] for o in outs], axis=1) for k in OUT_KEYS}
    for s in range(streams):
        for f, w in enumerate(want[s]):
            assert out['id'][s, f].tolist() == w['id'], (what, s, f, out['id'][s, f], w['id'])
            assert out['missed'][s, f].tolist() == w['missed'], (what, s, f, out['missed'][s, f], w['missed'])
            assert int(out['count'][s, f]) == w['count'] and int(out['dropped'][s, f]) == w['dropped'], (what, s, f)
            if w['count'] < 0:
                assert not out['box'][s, f].any() and not out['score'][s, f].any() and not out['cls'][s, f].any()
                continue
            assert np.array_equal(_bits(out['box'][s, f]), _bits(boxes[s][f])), (what, s, f)
            assert np.array_equal(_bits(out['score'][s, f]), _bits(scores[s][f])), (what, s, f)
    _assert_state_equals(state, f32s, what)
    return want, out


@pytest.mark.parametrize('variant', ['4', '5iou', '5rot'])
def test_optimal_keeps_both_identities_where_greedy_starts_a_third(variant):
    """Detection A overlaps track 1 by 0.6 and track 2 by 0.5, detection B only track 1 (0.574): the optimal assignment keeps ids
    {1, 2}; the greedy walk on the same records gives A track 1, starts id 3 for B and lets track 2 coast."""
    want, out = _check_case(ac.ab_case(variant, 'optimal'), f'ab {variant} optimal')
    assert sorted(i for i in out['id'][0, 1].tolist() if i) == [1, 2] and out['missed'][0, 1].tolist() == [0, 0, -1, -1]
    want, out = _check_case(ac.ab_case(variant, 'greedy'), f'ab {variant} greedy')
    assert out['id'][0, 1].tolist() == [1, 2, 3, 0] and out['missed'][0, 1].tolist() == [0, 1, 0, -1]


@pytest.mark.parametrize('assign', ['greedy', 'optimal'])
def test_low_score_detections_continue_a_track_but_never_start_one(assign):
    """conf_thres 0.3, low_thres 0.1 (see _assoc_cases.bands_frames): the track that gets 0.2-score detections in frames 3 and 4
    has missed == 0 throughout and one id; a low detection is never born, does not continue a track with missed >= 2, is not
    offered a track that stage 1 took, and a detection below low_thres is ignored.  Without bands, on the records filtered at
    0.3, the track coasts."""
    want, out = _check_case(ac.bands_case(assign), f'bands {assign}')
    assert out['missed'][0, :, 0].tolist() == [0] * 6 and out['id'][0, :, 0].tolist() == [1] * 6
    assert out['missed'][0, :, 1].tolist() == [0, 0, 0, 1, 2, 0] and out['count'][0].tolist() == [3] * 6 and not out['id'][0, :, 3:].any()
    want, out = _check_case(ac.bands_case(assign, bands=False), f'filtered {assign}')
    assert out['missed'][0, :, 0].tolist() == [0, 0, 0, 1, 2, 0] and out['id'][0, :, 0].tolist() == [1] * 6


@pytest.mark.parametrize('assign', ['greedy', 'optimal'])
def test_the_assignment_never_crosses_classes(assign):
    want, out = _check_case(ac.classes_case(assign), f'classes {assign}')
    assert out['cls'][0, 1].tolist() == [0, 1, 0, 1] and out['missed'][0, 1].tolist() == [0, 0, 0, 0]


def test_130_tracks_and_70_detections_over_three_streams_and_two_launches():
    """More than 64 columns, several columns per lane, three wavefronts, dummy columns in use (five dropped detections per frame):
    streams 3, two frames per stream in one launch, the second launch continues the state of the first."""
    case = dict(width=4, match='iou', max_tracks=ac.GRID_MT, params=ac.GRID_PARAMS, assoc=dict(assign='optimal'), ties=0,
                frames=[ac.grid_frames(seed) for seed in (1, 2, 3)], expect=None)
    want, out = _check_case(case, 'grid', streams=3, launches=2)
    assert out['count'].tolist() == [[65, 130, 130, 130]] * 3 and out['dropped'].tolist() == [[0, 0, 5, 5]] * 3
    assert ((out['missed'][:, 2:] == 0).sum(axis=2) == 65).all()


@pytest.mark.parametrize('variant', ['4', '5'])
def test_exact_ties_go_to_the_lower_slot(variant):
    want, out = _check_case(ac.tie_case('optimal', variant), f'tie {variant}')
    assert out['missed'][0, 1].tolist() == [0, 1, -1, -1]


@pytest.mark.parametrize('assoc', [dict(assign='greedy'), dict(assign='greedy', **ac.BANDS), dict(assign='optimal'),
                                   dict(assign='optimal', **ac.BANDS)], ids=['greedy', 'greedy-bands', 'optimal', 'optimal-bands'])
def test_a_bad_class_frame_leaves_the_state_alone(assoc):
    want, out = _check_case(ac.bad_class_case(assoc), f'bad class {assoc}')
    assert int(out['count'][0, 1]) == -1 and out['missed'][0, 2].tolist() == [0, -1, -1, -1]      # matched after ONE prediction


def test_error_codes_of_the_new_entry_point():
    """The argument errors on device buffers: nothing is launched (the state and the outputs keep their bits), and a correct call
    returns 0."""
    from mydetection_amd import _lib, ops
    case = ac.ab_case('4', 'optimal')
    rec = torch.from_numpy(ref.pack_records(case['frames'], 4)).cuda()
    par = ops.track_params(ac.IMG_HW)
    state = ops.track_state(1, 4, 'cuda')
    out = {k: torch.full(shape, 7, dtype=dt, device='cuda') for k, (shape, dt) in
           dict(box=((1, 2, 4, 5), torch.float32), score=((1, 2, 4), torch.float32), cls=((1, 2, 4), torch.int64), id=((1, 2, 4), torch.int64),
                missed=((1, 2, 4), torch.int32), count=((1, 2), torch.int32), dropped=((1, 2), torch.int32)).items()}
    before = {k: v.clone() for k, v in out.items()}
    fresh = state.clone()
    lib = _lib.lib()

    def call(assoc, bw=4):
        code = lib.mydet_track_frames_assoc_f32(ops._ptr(rec), 2 * rec.shape[1], rec.shape[1], 1, 2, bw, ctypes.byref(par), 4, ops._ptr(state),
                                                *[ops._ptr(out[k]) for k in OUT_KEYS], ctypes.byref(assoc) if assoc is not None else None,
                                                ops._stream())
        torch.cuda.synchronize()
        return code

    def assoc(**kw):
        a = ops.track_assoc('optimal', 0.1, 0.3, 0.3)
        for k, v in kw.items():
            setattr(a, k, v)
        return a
    assert call(None) == -1 and call(assoc(assign=2)) == -1 and call(assoc(bands=2)) == -1 and call(assoc(bands=-1)) == -1
    assert call(assoc(high_thres=float('nan'))) == -1 and call(assoc(low_thres=float('inf'))) == -1
    assert call(assoc(low_match_thres=float('nan'))) == -1 and call(assoc(low_thres=0.3)) == -1 and call(assoc(low_thres=0.4)) == -1
    assert call(assoc(), bw=3) == -1
    assert torch.equal(state, fresh) and all(torch.equal(out[k], before[k]) for k in OUT_KEYS)
    for a in (assoc(), ops.track_assoc('optimal'), ops.track_assoc('greedy', 0.1, 0.3, 0.3), ops.track_assoc()):
        ops.track_reset_(state, 4)
        assert call(a) == 0
        assert out['id'][0, 0].tolist() == [1, 2, 0, 0] and not torch.equal(state, fresh)


@pytest.mark.parametrize('name', ['slot_reuse', 'rotated_match'])
def test_the_old_entry_point_is_the_new_one_with_greedy_and_one_band(name):
    """mydet_track_frames_f32 and mydet_track_frames_assoc_f32 with {GREEDY, bands 0} write identical outputs and state: the int32
    words are compared.  Thresholds in an assoc without bands are not read."""
    from mydetection_amd import ops
    case = tc.cases()[name]
    rec = torch.from_numpy(ref.pack_records(case['frames'], case['width'])).cuda()
    par = ops.track_params(tc.IMG_HW, case['match'], **case['params'])
    junk = ops.track_assoc()
    junk.high_thres, junk.low_thres, junk.low_match_thres = float('nan'), 5.0, -1.0
    results = []
    for assoc in (None, ops.track_assoc(), junk):
        state = ops.track_state(1, case['max_tracks'], 'cuda')
        out = ops.track_frames(rec, state, par, assoc=assoc)
        torch.cuda.synchronize()
        results.append([state.cpu().numpy()] + [out[k].cpu().numpy().view(np.int32) for k in OUT_KEYS])
    for other in results[1:]:
        assert all(np.array_equal(a, b) for a, b in zip(results[0], other))
    assert results[0][OUT_KEYS.index('id') + 1].any()


def test_predict_frames_with_an_optimal_two_stage_tracker():
    """Detector('rapid').predict_frames(frames, tracker=Tracker(assign='optimal', low_thres=0.05)) on the frames of
    test_gpu_track's model test: the post-process of the call runs at min(conf_thres, 0.05), the objects are the tracks that
    ops.track_frames gives by hand on those records with the call's conf_thres as high_thres and new_thres, every row has an
    obj_id, and a plain call with today's Tracker() is unchanged."""
    from mydetection_amd import ops, synth
    from mydetection_amd.api import Detector, Tracker
    from mydetection_amd.models.general import name_to_model
    m, cfg = name_to_model('rapid')
    m.load_state_dict(synth.make_state_dict(m.state_dict(), 'rapid'), strict=True)
    det = Detector(model_and_cfg=(m.eval().cuda(), cfg))
    H, W, B = 150, 200, 4
    conf, low = E2E_CONF, 0.05
    kw = dict(input_size=128, conf_thres=conf)
    base = _synthetic_frames(1, H, W, seed=90)[0]
    frames = np.stack([base, base, np.roll(base, 3, axis=1), np.roll(base, 6, axis=1)])
    tkw = dict(min_score=0.0005)
    # the records of the call: post-processed at the lower threshold, both bands in them
    (_, r_low), = det._frame_records(frames, _whole_records=True, **dict(kw, conf_thres=low))
    (_, r_high), = det._frame_records(frames, _whole_records=True, **kw)
    n_low, n_high = int(r_low['count'].sum()), int(r_high['count'].sum())
    assert n_low > n_high > 0, (n_low, n_high)
    trk = Tracker(assign='optimal', low_thres=low, **tkw)
    got = det.predict_frames(frames, tracker=trk, **kw)
    state = ops.track_state(1, 256, 'cuda')
    par = ops.track_params((H, W), 'rotated', new_thres=conf, **tkw)
    out = ops.track_frames(r_low, state, par, assoc=ops.track_assoc('optimal', low, conf, 0.3))
    torch.cuda.synchronize()
    assert torch.equal(trk.state, state) and len(got) == B
    total = 0
    for f, o in enumerate(got):
        keep = out['missed'][0, f] == 0
        assert o.obj_ids is not None and len(o.obj_ids) == len(o) == int(keep.sum()) and (o.obj_ids > 0).all()
        assert torch.equal(o.obj_ids, out['id'][0, f][keep]) and torch.equal(o.bboxes, out['box'][0, f][keep])
        assert torch.equal(o.scores, out['score'][0, f][keep]) and torch.equal(o.cats, out['cls'][0, f][keep])
        total += len(o)
    assert total > 0 and int(out['id'].max()) <= n_high                           # only high detections start tracks
    # today's Tracker(): the call's settings are untouched, the tracks are those of the entry point of old
    plain = Tracker(**tkw)
    got = det.predict_frames(frames, tracker=plain, **kw)
    state = ops.track_state(1, 256, 'cuda')
    out = ops.track_frames(r_high, state, par)
    torch.cuda.synchronize()
    assert torch.equal(plain.state, state)
    for f, o in enumerate(got):
        keep = out['missed'][0, f] == 0
        assert torch.equal(o.obj_ids, out['id'][0, f][keep]) and torch.equal(o.bboxes, out['box'][0, f][keep])
    untracked = det.predict_frames(frames, **kw)
    assert [len(o) for o in untracked] == r_high['count'].tolist() and all(o.obj_ids is None for o in untracked)



def _rows(outs, n_frames):
    """JSON hypothesis rows of the tracks with missed == 0, frame by frame (x, y, w, h boxes)."""
    rows = []
    for f in range(n_frames):
        for slot in np.flatnonzero(outs['missed'][f] == 0):
            cx, cy, w, h = (float(v) for v in outs['box'][f][slot][:4])
            rows.append({'image_id': f, 'category_id': 1, 'bbox': [cx - w / 2, cy - h / 2, w, h], 'track_id': int(outs['id'][f][slot]),
                         'score': float(outs['score'][f][slot])})
    return rows


def test_scored_the_two_stage_optimal_tracker_loses_no_identity_and_no_frame():
    """Two objects that pass close by each other over twelve frames, one with a two-frame score dip, scored by TrackEvaluator.
    Greedy without bands (on the records a post-process at 0.3 leaves): the id switches and misses the restatement predicts.
    Optimal with bands: idsw == 0 and fn == 0."""
    from mydetection_amd import ops
    from mydetection_amd.api import TrackEvaluator
    frames, truth = ac.crossing()
    n = len(frames)
    gt = {'images': [{'id': f} for f in range(n)], 'categories': [{'id': 1}],
          'annotations': [{'id': 2 * f + k, 'image_id': f, 'category_id': 1, 'person_id': k + 1,
                           'bbox': [b[0] - b[2] / 2, b[1] - b[3] / 2, b[2], b[3]]} for f in range(n) for k, b in enumerate(truth[f])]}
    params = dict(match_thres=0.25)
    modes = {'greedy': (dict(assign='greedy'), ac._filtered(frames, 0.3)),
             'optimal-bands': (dict(assign='optimal', low_thres=0.1, high_thres=0.3, low_match_thres=0.25), frames)}
    counts = {}
    for name, (assoc, fr) in modes.items():
        case = dict(width=4, match='iou', max_tracks=4, params=params, assoc=assoc, ties=0, frames=fr, expect=None)
        want, out = _check_case(case, f'crossing {name}')
        # the restatement's prediction: its own float32 boxes through the scorer's restatement
        f32 = aref.Stream(4, ref.Params(ac.IMG_HW, np.float32, match='iou', **params), **assoc)
        pred = {'missed': [], 'box': [], 'id': [], 'score': []}
        for r in ref.pack_records(fr, 4):
            o = f32.step(*ref.unpack_frame(r, 4))
            a = f32.arrays()
            pred['missed'].append(np.array(o['missed']))
            pred['box'].append(a['x'].T.copy())
            pred['id'].append(np.array(o['id']))
            pred['score'].append(a['score'].copy())
        e = _mot_ref.evaluate(_rows(pred, n), gt, 'coco', [0.5])
        predicted = dict(zip(('tp', 'fp', 'fn', 'idsw', 'frag'), (int(v) for v in e['counts'][0, 0])))
        ev = TrackEvaluator(gt, kind='coco', iou_thrs=(0.5,))
        ev.add_json(_rows({k: out[k][0] for k in ('missed', 'box', 'id', 'score')}, n))
        got = ev.result()['overall'][0]
        torch.cuda.synchronize()
        print(name, {k: got[k] for k in predicted}, 'predicted', predicted)
        assert {k: got[k] for k in predicted} == predicted, (name, got, predicted)
        counts[name] = predicted
    assert counts['optimal-bands']['idsw'] == 0 and counts['optimal-bands']['fn'] == 0 and counts['optimal-bands']['fp'] == 0
    assert counts['greedy'] == {'tp': 22, 'fp': 0, 'fn': 2, 'idsw': 2, 'frag': 1}, counts['greedy']
