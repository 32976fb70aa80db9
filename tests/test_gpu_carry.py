"""GPU tests of the key-frame carry (include/mydet.h: mydet_carry_records_rgb_u8 / _yuv420; csrc/carry.hip) and of keyframes= in
the frame methods of Detector.

The checker is tests/_carry_ref.py, the rule text in Python integers, which tests/test_carry_host.py holds to the known motions
of tests/_carry_cases.py.  After one float32 conversion of the box everything is integer arithmetic, so the records, how, offset,
sad and every word of the state equal the restatement with ==; no case is left out.  Only the last test runs a model."""
import functools

import numpy as np
import pytest
import torch

import _carry_cases as cases
import _carry_ref as ref

pytestmark = pytest.mark.gpu

GUARD, SENTINEL = 64, 0x5A5A5A5A


def _guarded(shape):
    """A contiguous int32 tensor of `shape` in the middle of a buffer of sentinels; returns (tensor, buffer)."""
    n = int(np.prod(shape))
    buf = torch.full((2 * GUARD + n,), SENTINEL, dtype=torch.int32, device='cuda')
    return buf[GUARD:GUARD + n].view(shape), buf


def _guards_stand(buf):
    return bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[-GUARD:] == SENTINEL).all())


def _run(image_of, L, keys, splits=None, layout=None, rot=False, shift=None, settings=None, want=None):
    """The kernels on S streams x F frames, in one call or in the calls `splits` names, against the restatement's one call.
    image_of(f0, n): what ops.carry_records takes first for frames f0 .. f0 + n - 1 of every stream.  L: int64 [S, F, H, W]; keys: per
    stream its key records in order.  Every output lies between guard words, which must stand.  Returns (the restatement's outputs,
    its streams, the device state)."""
    from mydetection_amd import ops
    settings = settings or cases.SETTINGS
    cfg, cset = ref.Settings(**settings), ops.carry_set(**settings)
    S, F = L.shape[:2]
    words = ref.REC_ROT_WORDS if rot else ref.REC_WORDS
    if want is None:
        streams = [ref.Stream() for _ in range(S)]
        want = ref.run(streams, L, keys, 0, cfg, rot, shift), streams
    (w_rec, w_how, w_off, w_sad), streams = want
    state = ops.carry_state(S, 'cuda')
    parts, lo, k_lo = [], 0, 0
    for n in splits or [F]:
        mask = ref.key_mask(lo % cfg.every, cfg.every, n)
        K = sum(mask)
        key = None if K == 0 else torch.from_numpy(np.stack([np.stack(rows[k_lo:k_lo + K]) for rows in keys]).reshape(S * K, words)).cuda()
        bufs = {name: _guarded(shape) for name, shape in (('records', (S * n, words)), ('how', (S, n, 512)), ('offset', (S, n, 512, 2)),
                                                         ('sad', (S, n, 512, 2)))}
        sh = None if shift is None else torch.from_numpy(np.ascontiguousarray(shift[:, lo:lo + n]).astype(np.int32)).cuda()
        res = ops.carry_records(image_of(lo, n), key, mask, state, cset, frames_per_stream=n, layout=layout, shift=sh,
                                out={k: bufs[k][0] for k in ('how', 'offset', 'sad')}, records=bufs['records'][0])
        torch.cuda.synchronize()
        assert all(_guards_stand(b) for _, b in bufs.values()), 'a guard word was written'
        assert res['records'].data_ptr() == bufs['records'][0].data_ptr()
        parts.append({k: res[k].cpu().numpy() for k in ('records', 'how', 'offset', 'sad')})
        lo, k_lo = lo + n, k_lo + K
    assert lo == F
    rec = np.concatenate([p['records'].reshape(S, -1, words) for p in parts], axis=1)
    how, off, sad = (np.concatenate([p[k] for p in parts], axis=1) for k in ('how', 'offset', 'sad'))
    assert np.array_equal(how, w_how), np.argwhere(how != w_how)[:8].tolist()
    assert np.array_equal(off, w_off), np.argwhere(off != w_off)[:8].tolist()
    assert np.array_equal(sad, w_sad), np.argwhere(sad != w_sad)[:8].tolist()
    assert np.array_equal(rec, w_rec), np.argwhere(rec != w_rec)[:8].tolist()
    got = state.cpu().numpy()
    want_state = np.stack([st.words() for st in streams])
    assert np.array_equal(got, want_state), np.argwhere(got != want_state)[:8].tolist()
    return (w_rec, w_how, w_off, w_sad), streams, state


def _rgb_image(frames):
    """frames uint8 [S, F, H, W, 3] on the host -> image_of for _run (a fresh contiguous device batch per call)."""
    S = frames.shape[0]
    return lambda f0, n: torch.from_numpy(np.ascontiguousarray(frames[:, f0:f0 + n]).reshape((S * n,) + frames.shape[2:])).cuda()


@functools.lru_cache(maxsize=None)
def _want(rot=False):
    """The restatement's one call on the cases, computed once and left unchanged: (outputs, streams)."""
    streams = [ref.Stream(), ref.Stream()]
    return ref.run(streams, ref.luma_rgb(cases.rgb_frames()), cases.key_records(rot), 0, ref.Settings(**cases.SETTINGS), rot), streams


@pytest.mark.parametrize('rot', [False, True], ids=['plain', 'rotated'])
def test_rgb_crop_view_equals_the_restatement(rot):
    """The cases, every `how` value among them, as a crop view at an odd byte offset of a larger buffer with a row pitch above 3 W:
    read in place through the strides, nothing around the frames or the outputs written."""
    from mydetection_amd import ops
    frames = cases.rgb_frames()
    S, F, H, W = frames.shape[:4]
    buf = torch.from_numpy(np.random.default_rng(3).integers(0, 256, (S * F, H + 6, W + 10, 3), dtype=np.uint8)).cuda()
    view = buf[:, 3:3 + H, 5:5 + W]
    view.copy_(torch.from_numpy(frames.reshape(S * F, H, W, 3)).cuda())
    assert ops.packed_pixels(view) and not view.is_contiguous()
    keep = buf.clone()
    (_, how, _, _), _, _ = _run(lambda f0, n: view, ref.luma_rgb(frames), cases.key_records(rot), rot=rot, want=_want(rot))
    assert torch.equal(buf, keep)                                    # read only
    assert sorted(set(how.ravel().tolist())) == list(range(7))


def _planes(layout, y8, pitch_pad, seed):
    """4:2:0 planes on the device for the 8-bit luma y8 [B, H, W] with random chroma, every plane a view of a buffer whose rows are
    pitch_pad samples longer; the six bits a 10-bit layout ignores are random, and its two low bits round.  Returns (planes, the
    stored Y words)."""
    rng = np.random.default_rng(seed)
    B, H, W = y8.shape
    ch, cw = (H + 1) // 2, (W + 1) // 2
    ten = layout in ('p010', 'i010')

    def store(v8):
        if not ten:
            return v8.astype(np.uint8)
        junk = rng.integers(0, 64, v8.shape).astype(np.uint16)
        v10 = np.minimum(1023, (v8.astype(np.uint16) << 2) + rng.integers(0, 4, v8.shape).astype(np.uint16))
        return ((v10 << 6) | junk if layout == 'p010' else v10 | (junk << 10)).view(np.int16)

    def padded(a):
        buf = torch.zeros(a.shape[:2] + (a.shape[2] + pitch_pad,) + a.shape[3:], dtype=torch.from_numpy(a).dtype).cuda()
        view = buf[:, :, :a.shape[2]]
        view.copy_(torch.from_numpy(a).cuda())
        return view

    y = store(y8)
    if layout in ('i420', 'yv12', 'i010'):
        chroma = [store(rng.integers(0, 256, (B, ch, cw))) for _ in range(2)]
    else:
        chroma = [store(rng.integers(0, 256, (B, ch, cw, 2)))]
    return [padded(y)] + [padded(c) for c in chroma], y


@pytest.mark.parametrize('layout,pad', [('nv12', 0), ('nv21', 8), ('i420', 6), ('yv12', 0), ('p010', 0), ('i010', 4)])
def test_every_420_layout_equals_the_restatement_on_its_own_luma(layout, pad):
    """The luma is the Y sample as 8 bits, whatever the chroma and the ignored bits hold; pitches above W take the sample loads."""
    frames = cases.rgb_frames()
    S, F, H, W = frames.shape[:4]
    y8 = frames[..., 1].reshape(S * F, H, W)
    planes, stored = _planes(layout, y8, pad, seed=5)
    L = ref.luma_y(stored, layout).reshape(S, F, H, W)
    if layout in ('p010', 'i010'):
        assert (L != y8.reshape(S, F, H, W)).any()                   # the 10-bit rule rounds some samples up
    by_stream = [[p.unflatten(0, (S, F)) for p in planes]]
    image_of = lambda f0, n: [p[:, f0:f0 + n].flatten(0, 1) for p in by_stream[0]]
    _, streams, _ = _run(image_of, L, cases.key_records(), layout=layout)
    assert streams[0].slots[0].status == ref.CARRIED


def test_counts_0_and_512_and_the_bad_class_marker():
    """512 tiny boxes, the bad-class marker (its row is copied as it is and nothing is carried) and an empty record."""
    frames = cases.rgb_frames()[:1]
    tiny = [[3 + 4 * (j % 32) + 0.25 * (j % 3), 2 + 6 * (j // 32) + 0.5 * (j % 2), 2 + j % 3, 3] for j in range(512)]
    bad = ref.record(tiny[:7], count=-1)
    keys = [[ref.record(tiny), bad, ref.record([])]]
    settings = dict(cases.SETTINGS, every=2)
    (rec, how, _, _), _, _ = _run(_rgb_image(frames), ref.luma_rgb(frames), keys, settings=settings)
    assert rec[0, :, 0].tolist()[::2] == [512, -1, 0] and rec[0, 3, 0] == 0 and rec[0, 5, 0] == 0 and 0 < rec[0, 1, 0] <= 512
    assert (rec[0, 2] == bad).all() and not how[0, 2:].any() and (how[0, 0] == 1).all()
    assert {ref.CARRIED, ref.FLAT} <= set(how[0, 1].tolist())


@pytest.mark.parametrize('cut', [1, 2, 3, 4, 5])
def test_two_calls_equal_one_call(cut):
    """Every split of the 6 frames, those inside an interval included: the second call loads the templates from the state."""
    frames = cases.rgb_frames()
    _run(_rgb_image(frames), ref.luma_rgb(frames), cases.key_records(), splits=[cut, cases.F - cut], want=_want())


def test_fresh_state_equals_a_reset_one_and_the_views():
    from mydetection_amd import ops
    frames = cases.rgb_frames()
    _, streams, state = _run(_rgb_image(frames), ref.luma_rgb(frames), cases.key_records(), want=_want())
    v = {k: t.cpu().numpy() for k, t in ops.carry_state_views(state).items()}
    assert v['status'].shape == (2, 512) and v['coarse'].shape == (2, 512, 16, 16) and v['patch'].shape == (2, 512, 32, 32)
    for name, (s, j) in cases.SLOTS.items():
        sl = streams[s].slots[j]
        assert v['status'][s, j] == sl.status and v['cell'][s, j] == sl.s and v['offset'][s, j].tolist() == sl.off, name
        assert np.array_equal(v['coarse'][s, j], sl.coarse) and np.array_equal(v['patch'][s, j], sl.patch), name
    assert int(state.count_nonzero()) > 0
    ops.carry_reset_(state)
    assert torch.equal(state, ops.carry_state(2, 'cuda')) and int(state.count_nonzero()) == 0


def test_every_1_records_equal_the_key_records():
    frames = cases.rgb_frames()[:, :2]
    keys = [[ref.record(cases.key_boxes(s, f)) for f in (0, 3)] for s in range(2)]
    (rec, how, off, sad), _, _ = _run(_rgb_image(frames), ref.luma_rgb(frames), keys, settings=dict(cases.SETTINGS, every=1))
    assert all((rec[s, f] == keys[s][f]).all() for s in range(2) for f in range(2))
    assert set(how.ravel().tolist()) == {0, 1} and not off.any() and not sad.any()


def test_a_jump_is_followed_with_the_shift_and_lost_without_it():
    sc, frames, keys, shift = cases.jump_scene()
    L = ref.luma_rgb(frames)
    (rec, how, off, _), _, _ = _run(_rgb_image(frames), L, keys, shift=shift)
    assert how[0, :, 0].tolist() == [1, 2, 2] and off[0, 1:, 0].tolist() == [[13, -8], [14, -7]]
    for f in (1, 2):
        assert rec[0, f, ref.REC_BBOX:ref.REC_BBOX + 4].view(np.float32).tolist() == [float(v) for v in sc.box('small', f)]
    (_, how, _, _), _, _ = _run(_rgb_image(frames), L, keys)
    assert how[0, :, 0].tolist() == [1, 4, 4]


def _ids(out):
    """Per frame the ids of the tracks with missed == 0."""
    ids, missed = out['id'].cpu().numpy()[0], out['missed'].cpu().numpy()[0]
    return [sorted(ids[f][missed[f] == 0].tolist()) for f in range(ids.shape[0])]


def test_a_reversal_between_key_frames_keeps_its_id_only_with_the_carry():
    """The scenario the feature is for, both ways on the tracker's outputs: with the carried records the track keeps one id and
    every in-between box is the truth; the same key records with empty in-between rows give a new id at the third key frame,
    because the blind prediction went on to the right."""
    from mydetection_amd import ops
    sc, frames, keys = cases.reversal_scene()
    (rec, how, _, _), _, _ = _run(_rgb_image(frames), ref.luma_rgb(frames), keys, settings=cases.REVERSAL_SETTINGS)
    assert how[0, :, 0].tolist() == [1, 2, 2, 2, 1, 2, 2, 2, 1]
    for f in range(9):
        box = rec[0, f, ref.REC_BBOX:ref.REC_BBOX + 4].view(np.float32)
        assert np.abs(box[:2] - np.array(sc.box('turner', f)[:2], np.float32)).max() <= 1.0 and box[2:].tolist() == [28.0, 28.0], f
    par = ops.track_params(cases.HW)
    carried = ops.track_frames(torch.from_numpy(rec[0]).cuda(), ops.track_state(1, 16, 'cuda'), par, max_tracks=16)
    assert _ids(carried) == [[1]] * 9
    sparse = np.zeros_like(rec[0])
    sparse[::4] = rec[0, ::4]
    blind = ops.track_frames(torch.from_numpy(sparse).cuda(), ops.track_state(1, 16, 'cuda'), par, max_tracks=16)
    ids = _ids(blind)
    assert ids[0] == [1] and ids[4] == [1] and ids[8] == [2] and all(ids[f] == [] for f in (1, 2, 3, 5, 6, 7))


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


def test_frame_methods_with_keyframes(detector):
    from mydetection_amd import ops
    from mydetection_amd.api import Appearance, Augment, CameraMotion, KeyFrames, Tiles, Tracker, Zones
    from mydetection_amd.api.detection import _Yuv420Frames
    det = detector
    hw = (150, 200)
    frames = _video(hw)
    kw = dict(input_size=128, conf_thres=0.001)
    tkw = dict(min_score=0.0005, max_tracks=64)

    # every = 1: the objects of the call without it
    plain = det.predict_frames(frames, tracker=Tracker(**tkw), **kw)
    one = KeyFrames(every=1)
    got = det.predict_frames(frames, tracker=Tracker(**tkw), keyframes=one, **kw)
    assert _same(got, plain) and sum(len(o) for o in got) > 0
    assert one.last['how'].shape == (1, 4, 512) and set(one.last['how'].unique().tolist()) <= {0, 1} and one.frames == 4

    # every = 2: the ops composition -- the key frames through _frame_records, the carry, the tracker
    def composed(key_rec, image, layout, trk):
        state = ops.carry_state(1, 'cuda')
        rec = ops.carry_records(image, key_rec, [True, False, True, False], state, ops.carry_set(every=2), layout=layout)
        parts = {k: rec.pop(k) for k in ('how', 'offset', 'sad')}
        rec['img_hw'] = [key_rec['img_hw'][0]] * 4
        return det._tracked_objects([(list(range(4)), rec)], hw, trk, False, kw['conf_thres']), state, parts

    kf, trk, trk2 = KeyFrames(every=2), Tracker(**tkw), Tracker(**tkw)
    got = det.predict_frames(frames, tracker=trk, keyframes=kf, **kw)
    (_, key_rec), = det._frame_records(frames[::2], _whole_records=True, **kw)
    want, state, parts = composed(key_rec, torch.from_numpy(frames).cuda(), None, trk2)
    assert _same(got, want) and torch.equal(trk.state, trk2.state) and torch.equal(kf.state, state)
    assert all(torch.equal(kf.last[k], parts[k]) for k in parts) and (kf.streams, kf.max_tracks, kf.img_hw, kf.frames) == (1, None, hw, 4)
    assert int((kf.last['how'][0, 1::2] >= 2).sum()) > 0 and not (kf.last['how'][0, 1::2] == 1).any()
    # Tracker.reset() leaves the carry state, KeyFrames.reset() clears it and the counter
    before = kf.state.clone()
    trk.reset()
    assert torch.equal(kf.state, before)
    kf.reset()
    assert int(kf.state.count_nonzero()) == 0 and kf.last is None and kf.frames == 0

    # two calls of 3 and 1 frames continue each other: the call of 4
    kf2, trk3 = KeyFrames(every=2), Tracker(**tkw)
    a = det.predict_frames(frames[:3], tracker=trk3, keyframes=kf2, **kw)
    b = det.predict_frames(frames[3:], tracker=trk3, keyframes=kf2, **kw)
    assert _same(a + b, want) and torch.equal(kf2.state, state) and torch.equal(trk3.state, trk2.state) and kf2.frames == 4

    # NV12: its own ops composition on the planes
    y = np.ascontiguousarray(frames[..., 1])
    uv = np.ascontiguousarray(frames[:, ::2, ::2, :2])
    kf, trk, trk2 = KeyFrames(every=2), Tracker(**tkw), Tracker(**tkw)
    got = det.predict_frames_nv12(y, uv, tracker=trk, keyframes=kf, **kw)
    (_, key_rec), = det._source_records([_Yuv420Frames(det, (y[::2], uv[::2]), 'nv12', 'bt601', False)],
                                        det._call_settings(dict(kw, _whole_records=True)))
    want, state, _ = composed(key_rec, (torch.from_numpy(y).cuda(), torch.from_numpy(uv).cuda()), 'nv12', trk2)
    assert _same(got, want) and torch.equal(trk.state, trk2.state) and torch.equal(kf.state, state)

    # with the other keywords, and through the other frame methods
    polygon = [[(-16, -16), (216, -16), (216, 166), (-16, 166)]]
    for extra in (dict(tiles=Tiles((96, 128), overlap=0.25)), dict(augment=Augment()), dict(motion=CameraMotion()), dict(appearance=Appearance()),
                  dict(zones=Zones(polygons=polygon)), dict(coasting=True)):
        kf = KeyFrames(every=2)
        objs = det.predict_frames(frames, tracker=Tracker(**tkw), keyframes=kf, **extra, **kw)
        assert len(objs) == 4 and kf.last['how'].shape == (1, 4, 512) and int((kf.last['how'][0, ::2] == 1).sum()) > 0, extra
    for method in (det.annotate_frames, det.redact_frames, det.crop_frames):
        kf = KeyFrames(every=2)
        objs, made = method(frames.copy(), tracker=Tracker(**tkw), keyframes=kf, **kw)
        assert len(objs) == 4 and kf.frames == 4 and made is not None

    # every error comes before any launch: the tracker stays unbound
    trk = Tracker(**tkw)
    with pytest.raises(TypeError, match='KeyFrames'):
        det.predict_frames(frames, tracker=trk, keyframes=2, **kw)
    with pytest.raises(ValueError, match='tracker='):
        det.predict_frames(frames, keyframes=KeyFrames(), **kw)
    with pytest.raises(TypeError, match='json'):
        det.frames_to_json(frames, [0, 1, 2, 3], keyframes=KeyFrames(), **kw)
    assert trk.state is None
    bound = KeyFrames(every=2)
    det.predict_frames(frames, tracker=Tracker(**tkw), keyframes=bound, **kw)
    other = Tracker(streams=2, **tkw)
    with pytest.raises(ValueError, match='bound to'):
        det.predict_frames(frames, tracker=other, keyframes=bound, **kw)
    assert other.state is None and bound.frames == 4
