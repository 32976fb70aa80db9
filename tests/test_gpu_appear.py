"""GPU tests of the appearance: the descriptor launch (mydet_appear_boxes_rgb_u8 / _yuv420) against the numpy restatement
tests/_appear_ref.py -- every byte of desc, == for every settled box and the settled rule of the restatement's docstring for the
others --, the tracker launch (mydet_track_frames_appear_f32) against the plain-Python restatement with == on every output, the
tracker state and the appearance state, the two scenarios the feature is for, asserted both ways, the edges of the rules, and the
Detector level."""
import numpy as np
import pytest
import torch

import _appear_cases as cases
import _appear_ref as ref
import _track_ref
import _yuv420_ref

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5A5


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _check_desc(got, frames, boxes, counts, what):
    """got uint16 [B, K, 128] against the restatement: == for a settled box, the settled rule otherwise."""
    want, info = ref.descriptors(frames, boxes, counts)
    assert got.shape == want.shape and got.dtype == np.uint16
    exact = loose = 0
    for b in range(boxes.shape[0]):
        for k in range(boxes.shape[1]):
            i = info[b][k]
            if i is None:
                assert not got[b, k].any(), (what, b, k)             # a row that is not a box: zeros
            elif i['u'] == 0:
                assert np.array_equal(got[b, k], want[b, k]), (what, b, k, boxes[b, k])
                exact += 1
            else:
                extra = got[b, k].astype(np.int64) - i['settled']
                assert (extra >= 0).all() and extra.sum() == i['u'] and not extra[~i['reach']].any(), (what, b, k, boxes[b, k], i['u'])
                loose += 1
    return exact, loose


def test_rgb_descriptors_equal_the_restatement_and_write_only_desc():
    """2 x 49 x 67 frames as a crop view of a larger buffer (a non-tight row pitch), the named rows and the random ones; desc
    inside a sentinel buffer: every byte of desc is compared, the bytes around it and the frames stay as they were."""
    from mydetection_amd import ops
    frames = cases.frames()
    boxes, counts = cases.boxes()
    big = torch.full((2, cases.H + 6, cases.W + 9, 3), 77, dtype=torch.uint8, device='cuda')
    view = big[:, 2:2 + cases.H, 5:5 + cases.W]
    view.copy_(_dev(frames))
    before = big.clone()
    K = boxes.shape[1]
    arena = torch.full((4096 + 2 * K * 128 + 4096,), SENTINEL, dtype=torch.uint16, device='cuda')
    out = arena[4096:4096 + 2 * K * 128].view(2, K, 128)
    got = ops.appear_boxes(view, _dev(boxes), counts=_dev(counts), out=out)
    assert got.data_ptr() == out.data_ptr()
    host = arena.cpu().numpy()
    assert (host[:4096] == SENTINEL).all() and (host[-4096:] == SENTINEL).all()
    assert torch.equal(big, before)
    exact, loose = _check_desc(host[4096:-4096].reshape(2, K, 128), frames, boxes, counts, 'rgb')
    assert exact >= 30 and loose >= 2
    # the contiguous copy and no counts (every row a box), and one frame [H,W,3] with [K,5] boxes
    all_rows = ops.appear_boxes(_dev(frames), _dev(boxes)).cpu().numpy()
    _check_desc(all_rows, frames, boxes, None, 'rgb, no counts')
    one = ops.appear_boxes(_dev(frames[1]), _dev(boxes[1])).cpu().numpy()
    assert np.array_equal(one[0], all_rows[1])
    # 4-wide boxes: angle 0
    flat = boxes.copy()
    flat[..., 4] = 0
    assert torch.equal(ops.appear_boxes(_dev(frames), _dev(flat[..., :4].copy())), ops.appear_boxes(_dev(frames), _dev(flat)))


def test_counts_zero_full_and_bad_class():
    from mydetection_amd import ops
    frames = cases.frames()
    tiny = cases.tiny_boxes()
    got = ops.appear_boxes(_dev(frames[:1]), _dev(tiny), counts=_dev(np.array([512], np.int32))).cpu().numpy()
    exact, loose = _check_desc(got, frames[:1], tiny, np.array([512]), '512 rows')
    assert (exact, loose) == (512, 0) and got.sum() == 512 * 512
    boxes, _ = cases.boxes()
    for counts in ([0, 3], [-1, 24], [1000, -7]):
        c = np.array(counts, np.int32)
        got = torch.full((2, 24, 128), SENTINEL, dtype=torch.uint16, device='cuda')
        ops.appear_boxes(_dev(frames), _dev(boxes), counts=_dev(c), out=got)
        _check_desc(got.cpu().numpy(), frames, boxes, c, counts)


@pytest.mark.parametrize('layout', _yuv420_ref.LAYOUTS)
def test_every_420_layout_gives_the_descriptors_of_its_rgb_frames(layout):
    from mydetection_amd import ops
    H, W = 48, 66
    host = _yuv420_ref.random_planes(layout, 2, H, W, seed=17)
    planes = tuple(torch.from_numpy(p.view(np.int16) if p.dtype == np.uint16 else p).cuda() for p in host)
    before = [p.clone() for p in planes]
    boxes, counts = cases.boxes()
    for matrix, full in (('bt601', False), ('bt709', True)):
        rgb = ops.yuv420_to_rgb(planes, layout, matrix, full)
        want = ops.appear_boxes(rgb, _dev(boxes), counts=_dev(counts))
        got = ops.appear_boxes_yuv420(planes, layout, _dev(boxes), counts=_dev(counts), matrix=matrix, full_range=full)
        assert torch.equal(got.view(torch.int16), want.view(torch.int16)), (layout, matrix, full)
        assert int(got.view(torch.int16).count_nonzero()) > 0
    assert all(torch.equal(a, b) for a, b in zip(planes, before))
    if layout in ('nv12', 'i010'):                                     # and against the restatement, on the restated conversion
        frames = _yuv420_ref.to_rgb(host, layout, 'bt709', True)
        _check_desc(got.cpu().numpy(), frames, boxes, counts, layout)


def test_appear_records_reads_the_record_planes_in_place():
    from mydetection_amd import _lib, ops
    frames = cases.frames()
    boxes, counts = cases.boxes()
    for width in (4, 5):
        fr = [(boxes[b, :counts[b], :width], np.full(counts[b], 0.5, np.float32), np.zeros(counts[b], np.int64)) for b in range(2)] + [None]
        rec = _dev(_track_ref.pack_records(fr, width))
        views = ops.record_views(rec)
        three = np.concatenate([frames, frames[:1]])
        got = ops.appear_records(_dev(three), views).cpu().numpy()
        assert got.shape == (3, _lib.REC_TOPK, 128) and not got[2].any()              # the bad-class frame: zeros
        b5 = boxes.copy()
        if width == 4:
            b5[..., 4] = 0
        dense = np.zeros((3, 512, 5), np.float32)
        dense[:2, :24] = b5
        _check_desc(got, three, dense, np.array([counts[0], counts[1], -1]), f'records {width}')


# ---- the tracker ----

STATE_KEYS = ('x', 'v', 'pxx', 'pxv', 'pvv', 'score', 'cls', 'id', 'missed')


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def _launch(frames, descs, width, mt, match='iou', params=None, appear=None, assoc=None, shifts=None, cuts=None, with_appear=True):
    """The frames through ops.track_frames on fresh states, in calls of `cuts` frames: (outputs [F, ...], tracker state views,
    appearance state views), all numpy."""
    from mydetection_amd import ops
    rec = _dev(_track_ref.pack_records(frames, width))
    par = ops.track_params(cases.TRACK_HW, match, **(params or {}))
    tas = ops.track_assoc(**assoc) if assoc else None
    aset = ops.appear_set(**dict(dict(gate=None, reid=None, momentum=0.9, reach=2.0, update_thres=0.3), **(appear or {})))
    state, astate = ops.track_state(1, mt, 'cuda'), ops.appear_state(1, mt, 'cuda')
    d = _dev(descs)
    F = len(frames)
    outs, lo = [], 0
    for n in (cuts or [F]):
        sh = None if shifts is None else _dev(shifts[lo:lo + n]).view(1, n, 4)
        ap = (aset, d[lo:lo + n].contiguous(), astate) if with_appear else None
        outs.append(ops.track_frames(rec[lo:lo + n], state, par, assoc=tas, shift=sh, appear=ap))
        lo += n
    out = {k: torch.cat([o[k] for o in outs], dim=1)[0].cpu().numpy() for k in outs[0]}
    tv = {k: v[0].cpu().numpy() for k, v in ops.track_state_views(state, mt).items()}
    av = {k: v[0].cpu().numpy() for k, v in ops.appear_state_views(astate, mt).items()}
    return out, tv, av


def _assert_equals_restatement(out, tv, av, stream, outs, arrays, what):
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


VARIANTS = {'bw4': dict(width=4, match='iou'), 'bw5': dict(width=5, match='iou'), 'rot': dict(width=5, match='rotated')}
BANDS = dict(low_thres=0.2, high_thres=0.5, low_match_thres=0.3)


@pytest.mark.parametrize('mt', (64, 128, 512))
@pytest.mark.parametrize('bands', (False, True))
@pytest.mark.parametrize('variant', sorted(VARIANTS))
def test_tracker_equals_the_restatement(variant, bands, mt):
    """The busy scene (every `how`, a bad-class frame, templates that blend) with and without score bands and a camera shift:
    every output, the tracker state and the appearance state == the restatement, in one call and in two."""
    v = VARIANTS[variant]
    frames, descs = cases.busy(v['width'], low=bands, rot=variant != 'bw4')
    appear = dict(gate=0.3, reid=0.5, momentum=0.8, reach=2.0, update_thres=0.5)
    rappear = dict(gate=ref.level(0.3), reid=ref.level(0.5), alpha=ref.alpha_of(0.8), reach=2.0, update_thres=0.5)
    assoc = BANDS if bands else None
    shifts = np.zeros((len(frames), 4), np.int32)
    shifts[1], shifts[2] = (3, 1, 1, 9), (-2, 2, 0, 9)               # the second one is not valid: nothing moves
    for sh in (None, shifts):
        moved = [fr if fr is None or sh is None else (fr[0] + np.pad(np.cumsum(sh[:, :2] * sh[:, 2:3], axis=0)[f], (0, v['width'] - 2)).astype(np.float32),
                                                       fr[1], fr[2]) for f, fr in enumerate(frames)]
        stream, outs, arrays = ref.run(moved, descs, v['width'], cases.TRACK_HW, mt, params=dict(match=v['match']), appear=rappear,
                                       assoc=assoc, shifts=sh)
        m = stream.margins
        assert m['iou_thres'] >= 0.02 and m['iou_gap'] >= 0.02 and m['score'] >= 1e-3 and m['band'] >= 1e-3, m
        assert {h for o in outs for h in o['how']} >= ({-1, 0, 1, 3, 4} | ({2} if bands else set()))
        for cuts in (None, [3, len(frames) - 3]):
            out, tv, av = _launch(moved, descs, v['width'], mt, v['match'], appear=appear, assoc=assoc, shifts=sh, cuts=cuts)
            _assert_equals_restatement(out, tv, av, stream, outs, arrays, (variant, bands, mt, sh is not None, cuts))


@pytest.mark.parametrize('bands', (False, True))
@pytest.mark.parametrize('variant', sorted(VARIANTS))
def test_gate_and_reid_off_is_the_existing_entry_point(variant, bands):
    v = VARIANTS[variant]
    frames, descs = cases.busy(v['width'], low=bands, rot=variant != 'bw4')
    assoc = BANDS if bands else None
    new, tv, av = _launch(frames, descs, v['width'], 64, v['match'], assoc=assoc)
    old, tv0, _ = _launch(frames, descs, v['width'], 64, v['match'], assoc=assoc, with_appear=False)
    assert set(new) == set(old) | {'sim', 'how'}
    for k in old:
        assert np.array_equal(_bits(new[k]), _bits(old[k])), k
    for k in tv0:
        assert np.array_equal(_bits(tv[k]), _bits(tv0[k])), k
    assert av['has'].sum() > 0 and 3 not in new['how'] and int(new['id'].max()) > 6                # templates are kept all the same


def test_a_lost_track_comes_back_under_its_own_id():
    """Scenario (a): missed for 4 frames, back 1.5 box widths from its prediction.  The existing entry point gives it a new id;
    with reid it keeps its own and how == 3."""
    frames, descs = cases.lost_and_found()
    old, _, _ = _launch(frames, descs, 4, 64, with_appear=False)
    assert old['id'][3, 0] == 1 and old['id'][8, 1] == 2 and old['missed'][8, 1] == 0 and old['missed'][8, 0] == 5
    off, _, _ = _launch(frames, descs, 4, 64)
    assert np.array_equal(off['id'], old['id']) and off['how'][8, :2].tolist() == [0, 4]
    new, _, av = _launch(frames, descs, 4, 64, appear=dict(reid=0.6))
    assert new['id'][8, 0] == 1 and new['missed'][8, 0] == 0 and new['how'][8, 0] == 3 and new['sim'][8, 0] == ref.SIM_MAX
    assert (new['id'][:, 1:] == 0).all() and new['count'][8] == 1 and new['how'][9, 0] == 1
    stream, outs, arrays = ref.run(frames, descs, 4, cases.TRACK_HW, 64, appear=dict(reid=ref.level(0.6)))
    assert [o['id'] for o in outs] == new['id'].tolist() and [o['how'] for o in outs] == new['how'].tolist()


def test_two_objects_that_pass_each_other_keep_their_ids():
    """Scenario (b): the better-scored detection overlaps the other's prediction more.  The existing entry point swaps the ids;
    with the gate each track takes its own detection."""
    frames, descs = cases.crossing()
    old, _, _ = _launch(frames, descs, 4, 64, with_appear=False)
    new, _, _ = _launch(frames, descs, 4, 64, appear=dict(gate=0.3))
    assert old['id'][3, :2].tolist() == [1, 2] == new['id'][3, :2].tolist() and (old['missed'][3, :2] == 0).all() and (new['missed'][3, :2] == 0).all()
    # track 1 is RED (x = 200), track 2 BLUE (x = 224); the RED detection is at 214, the BLUE one at 208: a track that took the
    # other's detection has moved the wrong way
    # (the filter moves a track about 0.72 of the way to its detection: 205.8 / 216.8 when swapped, 210.1 / 212.4 when not)
    assert old['box'][3, 0, 0] < 208 and old['box'][3, 1, 0] > 214                                   # swapped: RED follows 208, BLUE 214
    assert 208 < new['box'][3, 0, 0] < 214 and 208 < new['box'][3, 1, 0] < 214                       # RED follows 214, BLUE 208
    assert new['sim'][3, :2].tolist() == [ref.SIM_MAX, ref.SIM_MAX] and new['how'][3, :2].tolist() == [1, 1]
    stream, outs, _ = ref.run(frames, descs, 4, cases.TRACK_HW, 64, appear=dict(gate=ref.level(0.3)))
    assert outs[3]['match'][:2] == [1, 0] and [o['sim'] for o in outs] == new['sim'].tolist()


def test_edges_of_the_rules():
    from mydetection_amd import ops
    RED, BLUE, MIXED = cases.RED, cases.BLUE, cases.MIXED
    box = (200.0, 200.0, 40.0, 60.0, 0.0)

    def fr(*rows):
        return cases._fr(list(rows), 4)

    # a track without a template (born by the entry point of old) passes the gate and is not re-identified
    rec = _dev(_track_ref.pack_records([fr((box, 0.9, 0))] * 2 + [fr()] * 2 + [fr(((290.0, 200.0, 40.0, 60.0, 0.0), 0.9, 0))], 4))
    d = _dev(cases.pack_desc([[RED], [BLUE], [], [], [RED]]))
    par, aset = ops.track_params(cases.TRACK_HW), ops.appear_set(gate=0.9, reid=0.1, update_thres=2.0)
    state, astate = ops.track_state(1, 64, 'cuda'), ops.appear_state(1, 64, 'cuda')
    ops.track_frames(rec[:1], state, par)
    out = ops.track_frames(rec[1:], state, par, appear=(aset, d[1:].contiguous(), astate))
    assert out['how'][0, :, 0].tolist() == [1, 0, 0, 0] and out['sim'][0, 0, 0] == 0 and out['how'][0, 3, 1] == 4      # gate passed; not re-identified
    assert ops.appear_state_views(astate, 64)['has'][0, :2].tolist() == [0, 1]         # update_thres 2: the match left has alone

    # a tie in S goes to the lower slot: two lost tracks with the same template, a detection between them
    left, right, mid = (200.0, 200.0, 40.0, 60.0, 0.0), (320.0, 200.0, 40.0, 60.0, 0.0), (260.0, 200.0, 40.0, 60.0, 0.0)
    frames = [fr((left, 0.9, 0), (right, 0.8, 0))] * 2 + [fr()] * 2 + [fr((mid, 0.9, 0))]
    descs = cases.pack_desc([[RED, RED], [RED, RED], [], [], [RED]])
    out, _, _ = _launch(frames, descs, 4, 64, appear=dict(reid=0.5))
    assert out['how'][4, :3].tolist() == [3, 0, -1] and out['sim'][4, 0] == ref.SIM_MAX
    # ... and the larger S wins over the lower slot
    descs = cases.pack_desc([[MIXED, RED], [MIXED, RED], [], [], [RED]])
    out, _, _ = _launch(frames, descs, 4, 64, appear=dict(reid=0.4))
    assert out['how'][4, :3].tolist() == [0, 3, -1] and out['sim'][4, 1] == ref.SIM_MAX

    # the reach boundary uses <=: m = 60 (the box height), reach 1.5 -> 90 px; the tracks stand still, so x[0] is 200 exactly
    for dx, found in ((90.0, True), (90.0078125, False)):
        frames = [fr((box, 0.9, 0))] * 2 + [fr()] * 2 + [fr(((200.0 + dx, 200.0, 40.0, 60.0, 0.0), 0.9, 0))]
        out, tv, _ = _launch(frames, cases.pack_desc([[RED], [RED], [], [], [RED]]), 4, 64, appear=dict(reid=0.5, reach=1.5))
        assert (out['how'][4, 0] == 3) == found and (out['how'][4, 1] == 4) == (not found), (dx, out['how'][4, :2])
        assert out['box'][3, 0, 0] == 200.0

    # a low-band match leaves the template alone (update_thres = the birth threshold), a high-band match moves it
    frames = [fr((box, 0.9, 0)), fr((box, 0.4, 0)), fr((box, 0.9, 0))]
    descs = cases.pack_desc([[RED], [BLUE], [MIXED]])
    out, _, av = _launch(frames, descs, 4, 64, appear=dict(momentum=0.5, update_thres=0.5), assoc=BANDS, cuts=[2])
    assert out['how'][:, 0].tolist() == [4, 2] and np.array_equal(av['tmpl'][:, 0], 256 * RED.astype(np.int32))
    out, _, av = _launch(frames, descs, 4, 64, appear=dict(momentum=0.5, update_thres=0.5), assoc=BANDS)
    assert out['how'][:, 0].tolist() == [4, 2, 1] and out['sim'][:, 0].tolist() == [-1, 0, ref.SIM_MAX // 2]
    assert np.array_equal(av['tmpl'][:, 0], 128 * RED.astype(np.int32) + 128 * MIXED.astype(np.int32))

    # a retire clears the template and the flag; the slot's next track starts from its own descriptor
    frames = [fr((box, 0.9, 0)), fr(), fr(), fr((box, 0.9, 0))]
    out, _, av = _launch(frames, cases.pack_desc([[RED], [], [], [BLUE]]), 4, 64, params=dict(max_missed=2), cuts=[3])
    assert out['how'][:, 0].tolist() == [4, 0, -1] and not av['has'].any() and not av['tmpl'].any()
    out, _, av = _launch(frames, cases.pack_desc([[RED], [], [], [BLUE]]), 4, 64, params=dict(max_missed=2))
    assert out['how'][3, 0] == 4 and out['id'][3, 0] == 2 and np.array_equal(av['tmpl'][:, 0], 256 * BLUE.astype(np.int32))


def test_c_entry_point_refuses_before_any_launch():
    """MYDET_E_UNSUPP for the optimal assignment and MYDET_E_BADARG for settings out of range, with real device buffers: the
    code comes back and every buffer stays as it was."""
    import ctypes
    from mydetection_amd import _lib, ops
    frames, descs = cases.crossing()
    rec, d = _dev(_track_ref.pack_records(frames, 4)), _dev(descs)
    state, astate = ops.track_state(1, 64, 'cuda'), ops.appear_state(1, 64, 'cuda')
    par = ops.track_params(cases.TRACK_HW)
    F = len(frames)
    outs = {k: torch.full(shape, 7, dtype=dt, device='cuda') for k, (shape, dt) in
            dict(box=((1, F, 64, 5), torch.float32), score=((1, F, 64), torch.float32), cls=((1, F, 64), torch.int64), id=((1, F, 64), torch.int64),
                 missed=((1, F, 64), torch.int32), count=((1, F), torch.int32), dropped=((1, F), torch.int32), sim=((1, F, 64), torch.int32),
                 how=((1, F, 64), torch.int32)).items()}
    s0, a0 = state.clone(), astate.clone()

    def call(assoc, aset):
        return _lib.lib().mydet_track_frames_appear_f32(rec.data_ptr(), rec.stride(0) * F, rec.stride(0), 1, F, 4, ctypes.byref(par), 64, state.data_ptr(),
                                                        *(outs[k].data_ptr() for k in ('box', 'score', 'cls', 'id', 'missed', 'count', 'dropped')),
                                                        ctypes.byref(assoc), None, ctypes.byref(aset), d.data_ptr(), astate.data_ptr(),
                                                        outs['sim'].data_ptr(), outs['how'].data_ptr(), None)
    assert call(ops.track_assoc('optimal'), ops.appear_set()) == -2
    bad = ops.appear_set()
    bad.alpha = 0
    assert call(ops.track_assoc(), bad) == -1
    torch.cuda.synchronize()
    assert torch.equal(state, s0) and torch.equal(astate, a0) and all(bool((t == 7).all()) for t in outs.values())
    with pytest.raises(ValueError, match='greedy'):
        ops.track_frames(rec, state, par, assoc=ops.track_assoc('optimal'), appear=(ops.appear_set(), d, astate))
    assert torch.equal(state, s0)


# ---- model level ----

@pytest.fixture(scope='module')
def detector():
    from mydetection_amd import synth
    from mydetection_amd.api import Detector
    from mydetection_amd.models.general import name_to_model
    m, cfg = name_to_model('rapid')
    m.load_state_dict(synth.make_state_dict(m.state_dict(), 'rapid'), strict=True)
    return Detector(model_and_cfg=(m.eval().cuda(), cfg))


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(o.bboxes, p.bboxes) and torch.equal(o.scores, p.scores) and torch.equal(o.cats, p.cats) and
                                    torch.equal(o.obj_ids, p.obj_ids) for o, p in zip(a, b))


def _video(hw=(150, 200), n=4, seed=4):
    rng = np.random.Generator(np.random.PCG64(seed))
    coarse = rng.integers(0, 256, size=(hw[0] // 10 + 2, hw[1] // 10 + 2, 3), dtype=np.uint8)
    big = np.repeat(np.repeat(coarse, 10, axis=0), 10, axis=1)
    return np.stack([np.ascontiguousarray(big[2 * f:2 * f + hw[0], 3 * f:3 * f + hw[1]]) for f in range(n)])


def test_frame_methods_with_appearance(detector):
    from mydetection_amd import ops
    from mydetection_amd.api import Appearance, CameraMotion, Tiles, Tracker
    det = detector
    hw = (150, 200)
    frames = _video(hw)
    kw = dict(input_size=128, conf_thres=0.001)
    tkw = dict(min_score=0.0005, max_tracks=64)

    # switched off: the objects of the call without it, the descriptors filled
    plain = det.predict_frames(frames, tracker=Tracker(**tkw), **kw)
    off = Appearance(gate=None, reid=None)
    got = det.predict_frames(frames, tracker=Tracker(**tkw), appearance=off, **kw)
    assert _same(got, plain) and sum(len(o) for o in got) > 0
    assert off.last['desc'].shape == (4, 512, 128) and int(off.last['desc'].view(torch.int16).count_nonzero()) > 0
    assert off.last['how'].shape == (1, 4, 64) and (off.streams, off.max_tracks, off.img_hw) == (1, 64, hw)

    # the defaults: the ops composition on the call's records
    ap, trk = Appearance(), Tracker(**tkw)
    got = det.predict_frames(frames, tracker=trk, appearance=ap, **kw)
    (_, r), = det._frame_records(frames, _whole_records=True, **kw)
    desc = ops.appear_records(torch.from_numpy(frames).cuda(), r)
    assert torch.equal(desc.view(torch.int16), ap.last['desc'].view(torch.int16))
    state, astate = ops.track_state(1, 64, 'cuda'), ops.appear_state(1, 64, 'cuda')
    par = ops.track_params(hw, 'rotated', new_thres=kw['conf_thres'], min_score=tkw['min_score'])
    want = ops.track_frames(r, state, par, appear=(ops.appear_set(0.3, 0.6, 0.9, 2.0, kw['conf_thres']), desc, astate))
    assert torch.equal(want['sim'], ap.last['sim']) and torch.equal(want['how'], ap.last['how'])
    assert torch.equal(state, trk.state) and torch.equal(astate, ap.state)
    keep = (want['missed'].view(4, 64) == 0)
    assert [len(o) for o in got] == keep.sum(dim=1).tolist()
    for f, o in enumerate(got):
        assert torch.equal(o.obj_ids, want['id'].view(4, 64)[f][keep[f]]) and torch.equal(o.bboxes, want['box'].view(4, 64, 5)[f][keep[f]])
    # Tracker.reset() leaves the templates, Appearance.reset() clears them
    trk.reset()
    assert int(ap.state.abs().sum()) > 0
    ap.reset()
    assert int(ap.state.abs().sum()) == 0 and ap.last is None

    # NV12: the call on the planes equals the RGB call on the converted frames
    y = np.ascontiguousarray(frames[..., 1])
    uv = np.ascontiguousarray(frames[:, ::2, ::2, :2])
    rgb = ops.yuv420_to_rgb((torch.from_numpy(y).cuda(), torch.from_numpy(uv).cuda()), 'nv12')
    a1, a2 = Appearance(), Appearance()
    o1 = det.predict_frames_nv12(y, uv, tracker=Tracker(**tkw), appearance=a1, **kw)
    o2 = det.predict_frames(rgb, tracker=Tracker(**tkw), appearance=a2, **kw)
    assert torch.equal(a1.last['desc'].view(torch.int16), a2.last['desc'].view(torch.int16)) and torch.equal(a1.state, a2.state)
    assert _same(o1, o2) and torch.equal(a1.last['how'], a2.last['how'])

    # with the other keywords, and through the other frame methods
    for extra in (dict(tiles=Tiles((96, 128), overlap=0.25)), dict(motion=CameraMotion()), dict(coasting=True)):
        ap = Appearance()
        objs = det.predict_frames(frames, tracker=Tracker(**tkw), appearance=ap, **extra, **kw)
        assert len(objs) == 4 and ap.last['how'].shape == (1, 4, 64) and int((ap.last['how'] == 4).sum()) > 0, extra
    ap = Appearance()
    objs, drawn = det.annotate_frames(frames.copy(), tracker=Tracker(**tkw), appearance=ap, **kw)
    assert len(objs) == 4 and ap.last is not None
    ap = Appearance()
    objs, chips = det.crop_frames(frames, tracker=Tracker(**tkw), appearance=ap, **kw)
    assert len(objs) == 4 and ap.last is not None

    # every error comes before any launch: the tracker stays unbound
    trk = Tracker(**tkw)
    with pytest.raises(TypeError, match='Appearance'):
        det.predict_frames(frames, tracker=trk, appearance='colour', **kw)
    with pytest.raises(ValueError, match='tracker='):
        det.predict_frames(frames, appearance=Appearance(), **kw)
    with pytest.raises(ValueError, match='greedy'):
        det.predict_frames(frames, tracker=Tracker(assign='optimal', **tkw), appearance=Appearance(), **kw)
    with pytest.raises(TypeError):
        det.frames_to_json(frames, [0, 1, 2, 3], appearance=Appearance(), **kw)
    bound = Appearance()
    det.predict_frames(frames, tracker=trk, appearance=bound, **kw)
    other = Tracker(min_score=0.0005, max_tracks=32)
    with pytest.raises(ValueError, match='bound to'):
        det.predict_frames(frames, tracker=other, appearance=bound, **kw)
    assert other.state is None
