"""GPU tests of the camera-motion estimator (include/mydet.h: mydet_motion_frames_rgb_u8 / _yuv420; csrc/motion.hip) and of the
tracker with the shift (mydet_track_frames_motion_f32).

The checker is tests/_motion_ref.py, the rule text in Python integers, which tests/test_motion_host.py holds to known shifts.
Everything the estimator does is integer arithmetic, so the shifts, the per-block rows and every field of the state equal the
restatement with ==; the tracker's state equals its float32 restatement bit for bit.  Only the last test runs a model."""
import functools

import numpy as np
import pytest
import torch

import _assoc_ref as aref
import _motion_ref as ref
import _track_ref
from test_gpu_track import _assert_state_equals, _bits

pytestmark = pytest.mark.gpu

SIZES = {'80x112': ((80, 112), 2, 4), '96x128': ((96, 128), 2, 8), '160x224': ((160, 224), 4, 4), '83x117': ((83, 117), 2, 4)}
MARGIN = 160


@functools.lru_cache(maxsize=None)
def _textures():
    return tuple(ref.texture(512, 640, seed) for seed in (7, 8, 9, 99))


def _rgb_crops(hw, shifts, seeds=(0, 1, 2)):
    """uint8 [len(shifts) + 1, H, W, 3]: crops of three textures (one per channel) that move together by `shifts`."""
    off = ref.offsets_of_shifts(shifts, MARGIN)
    return np.stack([ref.crops(_textures()[c], hw, off) for c in seeds], axis=-1)


def _grey_crops(hw, shifts, seed=0):
    return ref.crops(_textures()[seed], hw, ref.offsets_of_shifts(shifts, MARGIN))


def _run(image_of, lumas, hw, S, splits=None, layout=None, want=None, fill=None, **set_kw):
    """The kernels on S streams x F frames, in one call or in the calls `splits` names, against the restatement's one call.
    image_of(f0, n): what ops.motion_frames takes first for frames f0 .. f0 + n - 1 of every stream.  lumas: int64 [S, F, H, W].
    want: (shift, blocks, streams) of the restatement where the caller has them already (lumas is not read then).  fill: the
    outputs are passed in as out=, every word `fill` beforehand: what the kernels leave unwritten shows."""
    from mydetection_amd import ops
    if want is None:
        g = ref.Geometry(hw, set_kw.get('reduce'), set_kw.get('search', 8), set_kw.get('min_texture', 1024), set_kw.get('min_blocks'))
        streams = [ref.Stream(g) for _ in range(S)]
        want_shift, want_blocks = ref.run(streams, lumas)
    else:
        want_shift, want_blocks, streams = want
    F = want_shift.shape[1]
    mset = ops.motion_set(**set_kw)
    state = ops.motion_state(S, hw, mset, 'cuda')
    parts, lo = [], 0
    for n in splits or [F]:
        out = None
        if fill is not None:
            out = {'shift': torch.full((S, n, 4), fill, dtype=torch.int32, device='cuda'),
                   'blocks': torch.full((S, n, want_blocks.shape[2], 6), fill, dtype=torch.int32, device='cuda')}
        parts.append(ops.motion_frames(image_of(lo, n), state, mset, frames_per_stream=n, layout=layout, out=out))
        lo += n
    assert lo == F
    shift = torch.cat([p['shift'] for p in parts], dim=1).cpu().numpy()
    blocks = torch.cat([p['blocks'] for p in parts], dim=1).cpu().numpy()
    assert shift.dtype == np.int32 and shift.shape == want_shift.shape and blocks.shape == want_blocks.shape
    assert np.array_equal(shift, want_shift), (shift.tolist(), want_shift.tolist())
    assert np.array_equal(blocks, want_blocks), np.argwhere(blocks != want_blocks)[:8].tolist()
    _assert_motion_state(state, hw, mset, streams)
    return want_shift, state, mset, streams


def _assert_motion_state(state, hw, mset, streams):
    from mydetection_amd import ops
    got = {k: v.cpu().numpy() for k, v in ops.motion_state_views(state, hw, mset).items()}
    for s, st in enumerate(streams):
        assert int(got['seen'][s]) == st.seen
        assert np.array_equal(got['reduced'][s], st.reduced), ('reduced', s)
        assert np.array_equal(got['patches'][s], st.patches), ('patches', s)
    g = ops.motion_geometry(hw, mset)                                 # header, padding columns and tail are zero
    words = state.cpu().numpy()
    assert not words[:, 1:4].any()
    red = words[:, 4:4 + g['hr'] * g['wrp'] // 4].view(np.uint8).reshape(len(streams), g['hr'], g['wrp'])
    assert not red[:, :, g['wr']:].any() and not words[:, 4 + (g['hr'] * g['wrp'] + g['nb'] * g['P'] ** 2) // 4:].any()


def _rgb_image(frames, S):
    """frames uint8 [S, F, H, W, 3] on the host -> image_of for _run (a fresh contiguous device batch per call)."""
    return lambda f0, n: torch.from_numpy(np.ascontiguousarray(frames[:, f0:f0 + n]).reshape((S * n,) + frames.shape[2:])).cuda()


@pytest.mark.parametrize('size', sorted(SIZES))
def test_rgb_frames_equal_the_restatement(size):
    """The three sizes of the host test (contiguous frames: the wide loads of k = 2 and k = 4) and 83 x 117, where neither side
    is a multiple of k or 16 and the row pitch is odd (the byte loads): shifts up to the corner of the range."""
    hw, k, R = SIZES[size]
    m = R * k
    shifts = [(3, -5), (-m, m), (0, 0), (m - 1, 1 - m), (-1, 2)]
    frames = _rgb_crops(hw, shifts)[None]
    want, *_ = _run(_rgb_image(frames, 1), ref.luma_rgb(frames), hw, 1, reduce=k, search=R)
    assert want[0, 1:, :3].tolist() == [[dx, dy, 1] for dx, dy in shifts]


def test_rgb_crop_view_of_a_larger_buffer():
    """The frames are a crop view at an odd byte offset with a row pitch above 3 W: read in place through the strides."""
    from mydetection_amd import ops
    hw, k, R = SIZES['96x128']
    shifts = [(7, 4), (-9, -16)]
    frames = _rgb_crops(hw, shifts)[None]
    buf = torch.from_numpy(np.random.default_rng(3).integers(0, 256, (3, hw[0] + 6, hw[1] + 10, 3), dtype=np.uint8)).cuda()
    view = buf[:, 3:3 + hw[0], 5:5 + hw[1]]
    view.copy_(torch.from_numpy(frames[0]).cuda())
    assert ops.packed_pixels(view) and not view.is_contiguous()
    keep = buf.clone()
    _run(lambda f0, n: view[f0:f0 + n], ref.luma_rgb(frames), hw, 1, reduce=k, search=R)
    assert torch.equal(buf, keep)                                    # read only


def _planes(layout, y8, pitch_pad, seed):
    """4:2:0 planes on the device for the 8-bit luma y8 [B, H, W], random chroma, every plane a view of a buffer whose rows are
    pitch_pad samples longer; the six bits a 10-bit layout ignores are random."""
    rng = np.random.default_rng(seed)
    B, H, W = y8.shape
    ch, cw = (H + 1) // 2, (W + 1) // 2
    ten = layout in ('p010', 'i010')

    def store(v8):
        if not ten:
            return v8.astype(np.uint8)
        junk = rng.integers(0, 64, v8.shape).astype(np.uint16)
        v10 = v8.astype(np.uint16) << 2
        return ((v10 << 6) | junk if layout == 'p010' else v10 | (junk << 10)).view(np.int16)

    def padded(a):
        buf = torch.zeros(a.shape[:2] + (a.shape[2] + pitch_pad,) + a.shape[3:], dtype=torch.from_numpy(a).dtype).cuda()
        view = buf[:, :, :a.shape[2]]
        view.copy_(torch.from_numpy(a).cuda())
        return view

    y = store(y8)
    if layout in ('i420', 'i010'):
        chroma = [store(rng.integers(0, 256, (B, ch, cw))) for _ in range(2)]
    else:
        chroma = [store(rng.integers(0, 256, (B, ch, cw, 2)))]
    return [padded(y)] + [padded(c) for c in chroma], y


@pytest.mark.parametrize('layout,pad', [('nv12', 8), ('nv12', 0), ('i420', 6), ('p010', 0), ('i010', 4)])
def test_yuv420_planes_equal_the_restatement(layout, pad):
    """NV12 (pitch W + 8 and packed: wide loads) and I420 (pitch W + 6: sample loads) with pitches above W; P010 and I010: the
    luma is the Y sample as 8 bits, whatever the chroma and the ignored bits hold."""
    hw, k, R = SIZES['96x128']
    shifts = [(5, -3), (-16, 16), (2, 9)]
    y8 = _grey_crops(hw, shifts)
    planes, stored = _planes(layout, y8, pad, seed=11)
    lumas = ref.luma_y(stored, layout)[None]
    assert np.array_equal(lumas[0], y8)
    want, *_ = _run(lambda f0, n: [p[f0:f0 + n] for p in planes], lumas, hw, 1, layout=layout, reduce=k, search=R)
    assert want[0, 1:, :3].tolist() == [[dx, dy, 1] for dx, dy in shifts]


def _two_streams(hw):
    a = _rgb_crops(hw, [(4, 1), (-6, 8)])
    b = _rgb_crops(hw, [(-3, -7), (16, 0)], seeds=(2, 0, 3))
    return np.stack([a, b])


def test_two_streams_of_three_frames_with_their_own_shifts():
    hw, k, R = SIZES['96x128']
    frames = _two_streams(hw)
    want, *_ = _run(_rgb_image(frames, 2), ref.luma_rgb(frames), hw, 2, reduce=k, search=R)
    assert want[:, 1:, :3].tolist() == [[[4, 1, 1], [-6, 8, 1]], [[-3, -7, 1], [16, 0, 1]]]


@pytest.mark.parametrize('splits', [[1, 2], [2, 1], [1, 1, 1]])
def test_split_calls_equal_one_call(splits):
    """Calls of F1 and F2 frames leave exactly the outputs and the state of one call of F1 + F2: the first frame of a later call
    is matched against the reduced luma and the patches the state kept."""
    hw, k, R = SIZES['96x128']
    frames = _two_streams(hw)
    _run(_rgb_image(frames, 2), ref.luma_rgb(frames), hw, 2, splits=splits, reduce=k, search=R)


def test_flat_frames_and_a_scene_cut_report_no_motion():
    hw, k, R = SIZES['96x128']
    flat = np.full((1, 3) + hw + (3,), 90, np.uint8)
    want, *_ = _run(_rgb_image(flat, 1), ref.luma_rgb(flat), hw, 1, reduce=k, search=R)
    assert want[0].tolist() == [[0, 0, 0, 0]] * 3
    cut = np.concatenate([_rgb_crops(hw, [(6, -2)]), _rgb_crops(hw, [(-4, 5)], seeds=(3, 3, 1))])[None]
    want, *_ = _run(_rgb_image(cut, 1), ref.luma_rgb(cut), hw, 1, reduce=k, search=R)
    assert want[0, :, :3].tolist() == [[0, 0, 0], [6, -2, 1], [0, 0, 0], [-4, 5, 1]] and want[0, 2, 3] < 2


def test_search_16():
    hw = (96, 128)
    shifts = [(32, -32), (-31, 17)]
    frames = _rgb_crops(hw, shifts)[None]
    want, *_ = _run(_rgb_image(frames, 1), ref.luma_rgb(frames), hw, 1, reduce=2, search=16)
    assert want[0, 1:, :3].tolist() == [[dx, dy, 1] for dx, dy in shifts]


def test_default_settings_and_reset():
    """reduce=None resolves by frame size (k = 2 here); after a reset the next frame has no previous one."""
    from mydetection_amd import ops
    hw = (96, 128)
    frames = _rgb_crops(hw, [(3, 3), (-2, 6)])[None]
    lumas = ref.luma_rgb(frames)
    want, state, mset, streams = _run(_rgb_image(frames, 1), lumas, hw, 1)
    ops.motion_reset_(state, hw, mset)
    assert int(state.abs().sum()) == 0
    again = ops.motion_frames(_rgb_image(frames, 1)(0, 3), state, mset)
    assert np.array_equal(again['shift'].cpu().numpy(), want) and again['shift'][0, 0].tolist() == [0, 0, 0, 0]
    _assert_motion_state(state, hw, mset, streams)
    with pytest.raises(ValueError, match='streams'):
        ops.motion_frames(_rgb_image(frames, 1)(0, 3), ops.motion_state(2, hw, mset, 'cuda'), mset)
    with pytest.raises(ValueError, match='state'):
        ops.motion_frames(_rgb_image(frames, 1)(0, 3), state, ops.motion_set(search=16))   # another block grid: another state


# ---- the tracker with the shift ----

VARIANTS = {'greedy': ({}, {}), 'still_frame': (dict(still=4), {}), 'width5': (dict(width=5), {}),
            'optimal_low_band': (dict(low_from=3), dict(assign='optimal', low_thres=0.3, high_thres=0.6, low_match_thres=0.3))}


@pytest.mark.parametrize('variant', sorted(VARIANTS))
def test_tracker_with_the_shift_keeps_its_identities(variant):
    """Three boxes of about 24 px under frame shifts that alternate between (+20, -12) and (-18, +14): with the shift the ids
    persist over all frames and outputs and state equal the float32 restatement bit for bit (in one launch and in two); without
    it, on the same records, every track is lost at the first jerk and new ids appear."""
    from mydetection_amd import ops
    kw, assoc = VARIANTS[variant]
    width = kw.get('width', 4)
    frames, shifts = ref.tracker_scenario(**kw)
    s64, o64, _ = ref.run_tracker(frames, shifts, width, np.float64, assoc=assoc)
    assert aref.margins_hold(s64), s64.margins
    s32, o32, a32 = ref.run_tracker(frames, shifts, width, np.float32, assoc=assoc)
    rec = torch.from_numpy(_track_ref.pack_records(frames, width)).cuda()
    par = ops.track_params(ref.TRACK_HW, 'iou')
    tas = ops.track_assoc(**assoc) if assoc else None
    dshift = torch.from_numpy(shifts).cuda().view(1, -1, 4)
    F = len(frames)
    for cuts in ([F], [3, F - 3]):
        state = ops.track_state(1, 16, 'cuda')
        outs, lo = [], 0
        for n in cuts:
            outs.append(ops.track_frames(rec[lo:lo + n], state, par, assoc=tas, shift=dshift[:, lo:lo + n].contiguous()))
            lo += n
        out = {k: torch.cat([o[k] for o in outs], dim=1).cpu().numpy() for k in ('box', 'score', 'id', 'missed', 'count', 'dropped')}
        for f, (w64, w32) in enumerate(zip(o64, o32)):
            assert all(w64[k] == w32[k] for k in ('id', 'missed', 'count', 'dropped', 'match'))
            assert out['id'][0, f].tolist() == w32['id'] and out['missed'][0, f].tolist() == w32['missed'], (variant, f, out['id'][0, f])
            assert int(out['count'][0, f]) == w32['count'] == 3 and int(out['dropped'][0, f]) == 0
            assert out['id'][0, f, :3].tolist() == [1, 2, 3] and out['missed'][0, f, :3].tolist() == [0, 0, 0]
            assert np.array_equal(_bits(out['box'][0, f]), _bits(a32[f]['x'].T.copy())), (variant, f)
            assert np.array_equal(_bits(out['score'][0, f]), _bits(a32[f]['score'])), (variant, f)
        _assert_state_equals(state, [s32], variant)
    # the same records without the shift: the behaviour the shift is there to end
    state = ops.track_state(1, 16, 'cuda')
    plain = ops.track_frames(rec, state, par, assoc=tas)
    assert int(plain['id'].max()) > 3
    # shift = None is the entry point of old, bit for bit
    state2 = ops.track_state(1, 16, 'cuda')
    zero = torch.zeros_like(dshift)
    same = ops.track_frames(rec, state2, par, assoc=tas, shift=zero)  # valid = 0 everywhere: nothing moves
    assert all(torch.equal(plain[k], same[k]) for k in plain) and torch.equal(state, state2)
    with pytest.raises(ValueError, match='shift'):
        ops.track_frames(rec, state2, par, shift=zero[:, :2].contiguous())


# ---- model level ----

def test_frame_methods_with_motion():
    """Detector('rapid').predict_frames(frames, tracker=, motion=): on repeated identical frames every shift is (0, 0, 1) and the
    objects are bit for bit those of the call without motion=; on shifted crops motion.last['shift'] holds the true shifts, also
    through predict_frames_nv12, two calls continue from the state, and the other keywords and frame methods take motion= too."""
    from mydetection_amd import synth
    from mydetection_amd.api import CameraMotion, Detector, Tiles, Tracker, Zones
    from mydetection_amd.models.general import name_to_model
    m, cfg = name_to_model('rapid')
    m.load_state_dict(synth.make_state_dict(m.state_dict(), 'rapid'), strict=True)
    det = Detector(model_and_cfg=(m.eval().cuda(), cfg))
    hw, B = (150, 200), 4
    kw = dict(input_size=128, conf_thres=0.001)
    tkw = dict(min_score=0.0005)

    def same(a, b):
        return len(a) == len(b) and all(torch.equal(o.bboxes, p.bboxes) and torch.equal(o.scores, p.scores) and torch.equal(o.cats, p.cats) and
                                        torch.equal(o.obj_ids, p.obj_ids) for o, p in zip(a, b))

    still = np.repeat(_rgb_crops(hw, []), B, axis=0)
    plain = det.predict_frames(still, tracker=Tracker(**tkw), **kw)
    motion, trk = CameraMotion(), Tracker(**tkw)
    got = det.predict_frames(still, tracker=trk, motion=motion, **kw)
    shift = motion.last['shift'].cpu().numpy()
    assert shift.shape == (1, B, 4) and shift[0, 0].tolist() == [0, 0, 0, 0] and shift[0, 1:, :3].tolist() == [[0, 0, 1]] * (B - 1)
    assert same(got, plain) and sum(len(o) for o in got) > 0
    assert (motion.streams, motion.img_hw) == (1, hw) and int(motion.state[0, 0]) == 1
    trk.reset()
    assert int(motion.state[0, 0]) == 1                              # Tracker.reset() does not touch the estimator
    motion.reset()
    assert int(motion.state.abs().sum()) == 0 and motion.last is None

    shifts = [(9, -4), (-12, 7), (3, 16), (-5, -5), (1, 0)]
    moving = _rgb_crops(hw, shifts)                                  # 6 frames: two streams of three, or two calls
    motion = CameraMotion()
    det.predict_frames(moving, tracker=Tracker(streams=2, **tkw), motion=motion, **kw)
    assert motion.last['shift'].cpu().numpy()[:, :, :3].tolist() == [[[0, 0, 0], [9, -4, 1], [-12, 7, 1]], [[0, 0, 0], [-5, -5, 1], [1, 0, 1]]]
    motion, trk = CameraMotion(), Tracker(**tkw)
    det.predict_frames(moving[:2], tracker=trk, motion=motion, **kw)
    det.predict_frames(moving[2:], tracker=trk, motion=motion, **kw)
    assert motion.last['shift'].cpu().numpy()[0, :, :3].tolist() == [[dx, dy, 1] for dx, dy in shifts[1:]]
    with pytest.raises(ValueError, match='bound to'):
        det.predict_frames(moving, tracker=Tracker(streams=2, **tkw), motion=motion, **kw)

    y = np.ascontiguousarray(ref.luma_rgb(moving).astype(np.uint8))
    uv = np.full((len(y), hw[0] // 2, hw[1] // 2, 2), 128, np.uint8)
    motion = CameraMotion()
    det.predict_frames_nv12(y, uv, tracker=Tracker(**tkw), motion=motion, **kw)
    assert motion.last['shift'].cpu().numpy()[0, :, :3].tolist() == [[0, 0, 0]] + [[dx, dy, 1] for dx, dy in shifts]

    # motion= changes what the tracker does on moving frames and nothing else: with an estimator that never reports (a huge
    # min_texture: every frame valid = 0) the objects are those of the plain call, under every other keyword
    off = dict(min_texture=(1 << 24) - 1)
    left = [[(0, 0), (100, 0), (100, 150), (0, 150)]]
    for extra in (lambda: dict(tiles=Tiles((96, 128), overlap=0.25)), lambda: dict(coasting=True), lambda: dict(zones=Zones(polygons=left))):
        ref_objs = det.predict_frames(moving, tracker=Tracker(**tkw), **extra(), **kw)
        motion = CameraMotion(**off)
        objs = det.predict_frames(moving, tracker=Tracker(**tkw), motion=motion, **extra(), **kw)
        assert same(objs, ref_objs) and not motion.last['shift'][:, :, :3].any()
    motion = CameraMotion()
    objs, drawn = det.annotate_frames(moving, tracker=Tracker(**tkw), motion=motion, **kw)
    assert motion.last['shift'].cpu().numpy()[0, 1:, :3].tolist() == [[dx, dy, 1] for dx, dy in shifts] and drawn.shape == moving.shape
    want = det.predict_frames(moving, tracker=Tracker(**tkw), motion=CameraMotion(), **kw)
    assert same(objs, want)
