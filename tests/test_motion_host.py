"""Host tests of the camera-motion rules (include/mydet.h: mydet_motion_frames_rgb_u8) on their Python restatement
(tests/_motion_ref.py), of the tracker with the shift in float64 against float32, and of the argument errors of CameraMotion and
motion= -- no GPU.  tests/test_gpu_motion.py holds the kernels to the same restatement with ==."""
import functools

import numpy as np
import pytest
import torch

import _assoc_ref as aref
import _motion_ref as ref

SIZES = {'80x112': ((80, 112), 2, 4), '96x128': ((96, 128), 2, 8), '160x224': ((160, 224), 4, 4)}


def _shifts(k, R):
    m = R * k
    return [(0, 0), (1, 0), (0, -1), (-1, 1), (3, -5), (-7, 3), (m, m), (-m, -m), (m, -m), (m - 1, 1 - m)]


@functools.lru_cache(maxsize=None)
def _texture(seed=7):
    return ref.texture(512, 640, seed)


def _pair(hw, shift, noise, seed=0):
    """Two crops of the texture whose true shift is `shift`, the second with +-noise grey levels added: lumas int64 [2, H, W]."""
    fr = ref.crops(_texture(), hw, ref.offsets_of_shifts([shift], 160)).astype(np.int64)
    if noise:
        fr[1] = np.clip(fr[1] + np.random.default_rng(seed).integers(-noise, noise + 1, fr[1].shape), 0, 255)
    return fr


def _estimate(lumas, g):
    st = ref.Stream(g)
    return [st.step(L) for L in lumas]


@pytest.mark.parametrize('noise', [0, 2])
@pytest.mark.parametrize('size', sorted(SIZES))
def test_integer_shifts_are_recovered_exactly(size, noise):
    """Crops of one smoothed-noise texture: every shift up to R k in either direction -- zero, one pixel, no multiple of k, the
    range's corners, one short of it -- comes back exactly, with every block valid."""
    hw, k, R = SIZES[size]
    g = ref.Geometry(hw, k, R)
    assert g.nb == 6
    for i, d in enumerate(_shifts(k, R)):
        (first, _), (shift, blocks) = _estimate(_pair(hw, d, noise, seed=i), g)
        assert first.tolist() == [0, 0, 0, 0]
        assert shift.tolist() == [d[0], d[1], 1, 6], (size, noise, d, shift.tolist(), blocks.tolist())


def test_luma_and_reduction_follow_the_formulas():
    rgb = np.array([[[255, 255, 255], [0, 0, 0], [255, 0, 0], [0, 255, 0], [0, 0, 255], [10, 200, 30]]], np.uint8)
    assert ref.luma_rgb(rgb).tolist() == [[255, 0, 77, 149, 29, (770 + 30000 + 870 + 128) >> 8]]
    words = np.array([0, 64 << 6, 940 << 6, 1023 << 6], np.uint16)
    assert ref.luma_y(words, 'p010').tolist() == [0, 16, 235, 255] and ref.luma_y(words >> 6, 'i010').tolist() == [0, 16, 235, 255]
    g = ref.Geometry((83, 117), 2, 4)
    assert (g.hr, g.wr, g.nby, g.nbx, g.P, g.min_blocks) == (41, 58, 2, 3, 16, 2)
    L = np.arange(83 * 117).reshape(83, 117) % 251
    r = ref.reduce_luma(L, g)
    assert r.shape == (41, 58) and r[40, 57] == (L[80, 114] + L[80, 115] + L[81, 114] + L[81, 115] + 2) >> 2
    assert ref.Geometry((1080, 1920)).k == 4 and ref.Geometry((2160, 3840)).k == 8 and ref.Geometry((1024, 600)).k == 2
    assert ref.Geometry((1080, 1920)).min_blocks == 55
    assert ref.lower_median([5, 1, 3, 2]) == 2 and ref.lower_median([4]) == 4


def test_degenerate_inputs():
    """Flat frames and two unrelated textures report valid = 0; a third of the frame replaced by other content still gives the
    background's shift: the medians are the robustness."""
    hw, k, R = SIZES['96x128']
    g = ref.Geometry(hw, k, R)
    flat = np.full((2,) + hw, 90, np.int64)
    assert _estimate(flat, g)[1][0].tolist() == [0, 0, 0, 0]
    other = ref.texture(hw[0], hw[1], 99).astype(np.int64)
    shift, blocks = _estimate(np.stack([_pair(hw, (0, 0), 0)[0], other]), g)[1]
    assert shift[:3].tolist() == [0, 0, 0] and shift[3] < g.min_blocks, (shift, blocks)
    fr = _pair(hw, (5, -3), 0)
    fr[1, :, :hw[1] // 3] = other[:, :hw[1] // 3]
    shift, blocks = _estimate(fr, g)[1]
    assert shift[:3].tolist() == [5, -3, 1] and 2 <= shift[3] < 6, (shift, blocks)


def test_two_calls_equal_one_call():
    hw, k, R = SIZES['80x112']
    g = ref.Geometry(hw, k, R)
    shifts = [(3, -2), (-5, 4), (0, 7), (8, 8)]
    lumas = ref.crops(_texture(), hw, ref.offsets_of_shifts(shifts, 160)).astype(np.int64)[None]
    one = [ref.Stream(g)]
    want = ref.run(one, lumas)
    assert want[0][0, 1:, :3].tolist() == [[dx, dy, 1] for dx, dy in shifts]
    two = [ref.Stream(g)]
    a, b = ref.run(two, lumas[:, :2]), ref.run(two, lumas[:, 2:])
    assert np.array_equal(np.concatenate([a[0], b[0]], axis=1), want[0]) and np.array_equal(np.concatenate([a[1], b[1]], axis=1), want[1])
    assert two[0].seen == one[0].seen == 1 and np.array_equal(two[0].reduced, one[0].reduced) and np.array_equal(two[0].patches, one[0].patches)


def periodic_pair(hw, period, dx):
    """Two frames of a texture that repeats every `period` pixels along x, the second shifted by dx: shifts dx and dx -+ period
    have the same SAD (0)."""
    tile = ref.texture(hw[0] + 64, period, 5).astype(np.int64)
    wide = np.tile(tile, (1, hw[1] // period + 4))
    return np.stack([wide[32:32 + hw[0], 2 * period:2 * period + hw[1]], wide[32:32 + hw[0], 2 * period - dx:2 * period - dx + hw[1]]])


def test_equal_minima_take_the_smaller_motion():
    """A texture that repeats every 16 pixels (8 reduced pixels, R = 8): candidates -8, 0 and 8 tie at SAD 0 and 0 wins; shifted
    by 6, candidates 3 and -5 tie and 3 wins; along y nothing repeats."""
    hw, k, R = SIZES['96x128']
    g = ref.Geometry(hw, k, R)
    shift, blocks = _estimate(periodic_pair(hw, 16, 0), g)[1]
    assert shift.tolist() == [0, 0, 1, 6] and (blocks[:, 2] == 0).all()
    shift, blocks = _estimate(periodic_pair(hw, 16, 6), g)[1]
    assert shift.tolist() == [6, 0, 1, 6] and (blocks[:, 0] == 3).all() and (blocks[:, 2] == 0).all()
    shift, blocks = _estimate(periodic_pair(hw, 16, -6), g)[1]
    assert shift.tolist() == [-6, 0, 1, 6] and (blocks[:, 0] == -3).all()
    assert ref.best({(0, 1): 5, (0, -1): 5, (1, 0): 5, (-1, 0): 5, (1, 1): 4, (-1, -1): 4}, 1)[0] == (-1, -1)
    assert ref.best({(0, 1): 5, (0, -1): 5, (1, 0): 5, (-1, 0): 5}, 1)[0] == (-1, 0)


@pytest.mark.parametrize('variant', ['greedy', 'optimal_low_band', 'still_frame', 'width5'])
def test_shifted_tracker_float32_follows_float64(variant):
    """The tracker with the shift in the kernel's float32 operation order against float64: the same decisions in every frame,
    every decision away from its threshold, ids that persist through the jerks, and states within 16 ulp of a 512-pixel
    coordinate (a handful of roundings of at most half an ulp per frame, eight frames, gains below one).  Without the shift the
    same records lose every track at the first jerk."""
    kw = {'greedy': {}, 'optimal_low_band': dict(low_from=3), 'still_frame': dict(still=4), 'width5': dict(width=5)}[variant]
    assoc = dict(assign='optimal', low_thres=0.3, high_thres=0.6, low_match_thres=0.3) if variant == 'optimal_low_band' else {}
    width = kw.get('width', 4)
    frames, shifts = ref.tracker_scenario(**kw)
    s64, o64, a64 = ref.run_tracker(frames, shifts, width, np.float64, assoc=assoc)
    s32, o32, a32 = ref.run_tracker(frames, shifts, width, np.float32, assoc=assoc)
    assert aref.margins_hold(s64), s64.margins
    for f, (w, g) in enumerate(zip(o64, o32)):
        assert all(w[k] == g[k] for k in ('id', 'missed', 'count', 'dropped', 'match')), (variant, f, w, g)
        assert w['id'][:3] == [1, 2, 3] and w['missed'][:3] == [0, 0, 0] and w['count'] == 3, (variant, f, w)
        for name in ('x', 'v'):
            assert np.abs(a32[f][name].astype(np.float64) - a64[f][name]).max() <= 16 * 2.0 ** -15, (variant, f, name)
    if variant == 'still_frame':
        assert shifts[4].tolist() == [0, 0, 0, 0]
    _, plain, _ = ref.run_tracker(frames, None, width, np.float64, assoc=assoc)
    assert max(max(o['id']) for o in plain) > 3


def _meta_detector(name='yolov3_80'):
    from mydetection_amd.api import Detector
    from mydetection_amd.models.general import name_to_model
    with torch.device('meta'):
        m, cfg = name_to_model(name)
    return Detector(model_and_cfg=(m.eval(), cfg))


def test_argument_errors_before_any_device_is_touched():
    from mydetection_amd import _lib, ops
    from mydetection_amd.api import CameraMotion, Tracker
    for bad in (dict(reduce=3), dict(reduce=16), dict(search=3), dict(search=17), dict(search=8.5), dict(min_texture=-1), dict(min_blocks=0),
                dict(min_blocks=1025)):
        with pytest.raises(ValueError, match='motion_set'):
            CameraMotion(**bad)
    m = ops.motion_set()
    assert (m.reduce, m.search, m.min_texture, m.min_blocks) == (0, 8, 1024, 0)
    for hw, k, R in SIZES.values():
        geo = ops.motion_geometry(hw, ops.motion_set(k, R))
        g = ref.Geometry(hw, k, R)
        assert all(geo[n] == getattr(g, n) for n in ('k', 'R', 'hr', 'wr', 'nby', 'nbx', 'nb', 'P', 'min_blocks'))
        assert _lib.lib().mydet_motion_state_words(hw[0], hw[1], k, R) == geo['state_words']
    assert ops.motion_geometry((1080, 1920), m)['k'] == 4 == _lib.lib().mydet_motion_default_reduce(1080, 1920)
    assert ops.motion_geometry((2160, 3840), m)['k'] == 8 == _lib.lib().mydet_motion_default_reduce(2160, 3840)
    assert _lib.lib().mydet_motion_state_words(62, 128, 2, 8) == 0 and _lib.lib().mydet_motion_state_words(64, 64, 3, 8) == 0
    assert _lib.lib().mydet_motion_state_words(2160, 3840, 2, 8) == 0 and _lib.lib().mydet_motion_workspace_bytes(0, 96, 128, 2, 8) == 0
    with pytest.raises(ValueError, match='blocks'):
        ops.motion_geometry((2160, 3840), ops.motion_set(2))
    null = None
    lib = _lib.lib()
    assert lib.mydet_motion_reset(null, 1, 96, 128, 2, 8, null) == -1
    assert lib.mydet_motion_frames_rgb_u8(null, 2, 96, 128, 0, 384, 1, null, null, null, 0, null, null, null) == -1
    assert lib.mydet_motion_frames_yuv420(null, 2, 96, 128, 1, null, null, null, 0, null, null, null) == -1
    assert lib.mydet_track_frames_motion_f32(null, 0, 0, 1, 1, 4, null, 1, null, null, null, null, null, null, null, null, null, null, null) == -1
    with pytest.raises(TypeError, match='MotionSet'):
        ops.motion_frames(torch.zeros(2, 96, 128, 3, dtype=torch.uint8), torch.zeros(1, 8, dtype=torch.int32), 'set')
    with pytest.raises(RuntimeError):                                             # no CPU path
        ops.motion_state(1, (96, 128), m, 'cpu')

    det = _meta_detector()
    a = np.zeros((2, 96, 128, 3), np.uint8)
    for wrong in ('motion', True, 4):
        with pytest.raises(TypeError, match='CameraMotion'):
            det.predict_frames(a, tracker=Tracker(), motion=wrong)
    with pytest.raises(ValueError, match='tracker='):
        det.predict_frames(a, motion=CameraMotion())
    with pytest.raises(ValueError, match='2 \\* search \\+ 16'):
        det.predict_frames(np.zeros((2, 60, 128, 3), np.uint8), tracker=Tracker(), motion=CameraMotion())
    y, uv = np.zeros((2, 60, 128), np.uint8), np.zeros((2, 30, 64, 2), np.uint8)
    with pytest.raises(ValueError, match='2 \\* search \\+ 16'):
        det.predict_frames_nv12(y, uv, tracker=Tracker(), motion=CameraMotion())
    with pytest.raises(ValueError, match='tracker='):
        det.annotate_frames(a, motion=CameraMotion())
    bound = CameraMotion()
    bound.streams, bound.img_hw = 1, (48, 64)
    with pytest.raises(ValueError, match='bound to'):
        det.predict_frames(a, tracker=Tracker(), motion=bound)
    with pytest.raises(TypeError, match='json'):
        det.frames_to_json(a, [0, 1], motion=CameraMotion())
    assert 'does NOT' in CameraMotion.__doc__ and 'fixed camera' in CameraMotion.__doc__
