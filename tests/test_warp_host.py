"""Host tests of the similarity model of the camera-motion estimator: the restatement (tests/_warp_ref.py) against known
transforms, its integer rules against `math`, its invalid exits, and the argument rules of the bindings that need no device."""
import math

import numpy as np
import pytest

import _motion_ref as mref
import _warp_cases as cases
import _warp_ref as ref


# ---- pure shifts ----

@pytest.mark.parametrize('shift', [(7, -9), (0, 0), (-16, 16), (1, 0)])
def test_a_pure_integer_shift_is_the_identity_model_and_the_row_of_shift_mode(shift):
    hw = (320, 448) if shift == (7, -9) else (96, 128)
    g = mref.Geometry(hw, reduce=2, search=8)
    tex = mref.coarse_texture(hw[0] + 96, hw[1] + 96, 3)
    frames = mref.crops(tex, hw, mref.offsets_of_shifts([shift], 48)).astype(np.int64)
    out = ref.run([ref.Stream(g, ref.Fit())], frames[None])
    want_shift, _ = mref.run([mref.Stream(g)], frames[None])
    a, b, tx, ty, s_q, deg_q, valid, n_in = out['warp'][0, 1].tolist()
    assert (a, b, s_q, deg_q, valid) == (0, 0, 65536, 0, 1) and (tx, ty) == (shift[0] << 16, shift[1] << 16) and n_in == g.nb
    assert np.array_equal(out['shift'], want_shift) and out['shift'][0, 1].tolist() == [shift[0], shift[1], 1, g.nb]
    assert out['inliers'][0, 1].all() and not out['warp'][0, 0].any() and not out['inliers'][0, 0].any()
    # the pure-shift case of the table is the same scene through the warp of the case file
    if shift == (7, -9):
        _, w, _ = cases.want('scene', 'pure_shift')
        assert w['warp'][0, 1].tolist() == [0, 0, 7 << 16, -9 << 16, 65536, 0, 1, g.nb]


# ---- warped scenes ----

@pytest.mark.parametrize('name', ['turn_zoom_in', 'turn_zoom_out', 'turn_k4'])
def test_warped_scenes_are_recovered_within_the_corner_bound(name):
    c = cases.case('scene', name)
    g, out, _ = cases.want('scene', name)
    row = out['warp'][0, 1]
    truth = ref.true_model(*c['truths'][0][0])
    err = ref.corner_error(row, truth, c['hw'])
    print(name, 'corner error', err, 'row', row.tolist())
    assert row[6] == 1 and err <= cases.BOUND[c['hw']], err
    deg, zoom, _ = c['truths'][0][0]
    assert abs(row[5] / 65536 - deg) < 0.1 and abs(row[4] / 65536 - zoom) < 0.002
    assert row[7] == out['inliers'][0, 1].sum() >= 0.9 * out['shift'][0, 1, 3]
    # the whole-pixel shift is the model at the frame centre
    assert out['shift'][0, 1, :2].tolist() == [(int(row[2]) + 32768) >> 16, (int(row[3]) + 32768) >> 16]


def test_a_quarter_of_foreign_blocks_stays_within_the_same_bound():
    """27 of 117 blocks move by (-6, 7) instead: the pairing loses up to twice that share of its pairs, the medians hold, and
    the rounds drop the foreign blocks."""
    c = cases.case('outliers', 'quarter')
    g, out, _ = cases.want('outliers', 'quarter')
    row, inl = out['warp'][0, 1], out['inliers'][0, 1].reshape(g.nby, g.nbx)
    err = ref.corner_error(row, ref.true_model(*c['truths'][0][0]), c['hw'])
    print('outliers corner error', err, 'inliers', int(row[7]))
    assert row[6] == 1 and err <= cases.BOUND[c['hw']], err
    assert not inl[:, :2].any() and inl[:, 4:].all()                 # column 2 straddles the border of the region
    blocks = out['blocks'][0, 1].reshape(g.nby, g.nbx, 6)
    assert (blocks[:, :2, 4:] == (-6, 7)).all()


# ---- the integer rules ----

def test_isqrt_is_the_floor_of_the_root():
    rng = np.random.default_rng(0)
    values = [0, 1, 2, 3, 4, 65536 ** 2, 65536 ** 2 - 1, 65536 ** 2 + 1, (1 << 62) - 1] + [int(v) for v in rng.integers(0, 1 << 40, 2000)]
    for v in values:
        assert ref.isqrt(v) == math.isqrt(v), v


def test_the_arctangent_polynomial_is_within_8_units_of_math():
    worst = 0.0
    for u in list(range(-ref.U_MAX, ref.U_MAX + 1, 3)) + [ref.U_MAX]:
        d = ref.atan_deg_q(u)
        assert d == -ref.atan_deg_q(-u)
        worst = max(worst, abs(d - math.degrees(math.atan(u / 65536)) * 65536))
    print('worst', worst)
    assert worst <= 8.0
    assert ref.ATAN_C == tuple(round(180 / math.pi / d * 2 ** 24) for d in (1, 3, 5, 7))


def test_derived_integers_against_math():
    rng = np.random.default_rng(1)
    fit = ref.Fit(max_zoom=0.25, max_rotation=14.0)
    for _ in range(500):
        deg, zoom = rng.uniform(-13.5, 13.5), rng.uniform(0.8, 1.2)
        a, b = round((zoom * math.cos(math.radians(deg)) - 1) * 65536), round(zoom * math.sin(math.radians(deg)) * 65536)
        s_q, deg_q = ref.derived(a, b, fit)
        # the floor of u = (b << 16) / (65536 + a) is worth up to 180 / pi = 58 units of deg_q, the polynomial 8 more
        assert abs(s_q - math.hypot(65536 + a, b)) <= 1 and abs(deg_q - math.degrees(math.atan2(b, 65536 + a)) * 65536) <= 66


# ---- the invalid exits ----

def _lattice_blocks(g, model, noise=None):
    """Block rows whose vectors are the model at the block centres, rounded to whole pixels; every block valid."""
    blocks = np.zeros((g.nb, 6), np.int64)
    blocks[:, 3] = 1 << 20
    for b in range(g.nb):
        y0, x0 = g.origin(b)
        px, py = (x0 + 8) * g.k, (y0 + 8) * g.k
        mx, my = ref.apply_model(model, (g.H, g.W), px, py)
        blocks[b, 4:] = round(mx - px), round(my - py)
    if noise is not None:
        blocks[:, 4:] += noise
    return blocks


def test_the_fit_on_block_vectors_and_every_invalid_exit():
    g = mref.Geometry((320, 448), reduce=2, search=8)
    valid = list(range(g.nb))
    truth = ref.true_model(2.0, 1.03, (3.25, -1.5))
    m = ref.fit_model(g, _lattice_blocks(g, truth), valid, ref.Fit())
    assert m is not None and m[6] == g.nb
    assert ref.corner_error(m[:4], truth, (g.H, g.W)) < 0.3
    # a cap exceeded
    assert ref.fit_model(g, _lattice_blocks(g, truth), valid, ref.Fit(max_rotation=1.5)) is None
    assert ref.fit_model(g, _lattice_blocks(g, truth), valid, ref.Fit(max_zoom=0.02)) is None
    assert ref.fit_model(g, _lattice_blocks(g, truth), valid, ref.Fit(max_zoom=0.04, max_rotation=2.5)) is not None
    # no pair; one pair (all valid blocks in one pair position): two inliers at the most
    assert ref.fit_model(g, _lattice_blocks(g, truth), valid[:1], ref.Fit()) is None
    assert ref.fit_model(g, _lattice_blocks(g, truth), [5, 70], ref.Fit()) is None
    # fewer than 3 inliers: vectors that agree on no model
    rng = np.random.default_rng(2)
    assert ref.fit_model(g, _lattice_blocks(g, truth, rng.integers(-60, 61, (g.nb, 2))), valid, ref.Fit(tolerance=0.25)) is None
    # the guards behind the caps: a quarter turn (65536 + a <= 0 or |u| beyond the polynomial's domain)
    assert ref.derived(-65536, 65536, ref.Fit(max_zoom=0.25, max_rotation=14.0)) is None
    assert ref.derived(-70000, 60000, ref.Fit(max_zoom=0.25, max_rotation=14.0)) is None
    assert ref.derived(0, 20000, ref.Fit(max_zoom=0.25, max_rotation=14.0)) is None
    assert ref.derived(0, 16000, ref.Fit(max_zoom=0.25, max_rotation=14.0)) is not None


def test_random_block_vectors_with_outliers_and_invalid_blocks_at_the_1080p_geometry():
    """435 blocks, whole-pixel rounding, a fifth of the blocks invalid and a fifth of the rest with random vectors: the corner
    error stays below 0.3 px.  (The pairing loses up to twice the share of foreign blocks, so the start holds up to a
    quarter of them, not up to a half.)"""
    g = mref.Geometry((1080, 1920), reduce=4, search=8)
    assert g.nb == 435
    rng = np.random.default_rng(5)
    worst = 0.0
    for _ in range(20):
        truth = ref.true_model(rng.uniform(-3, 3), rng.uniform(0.96, 1.04), rng.uniform(-8, 8, 2))
        blocks = _lattice_blocks(g, truth)
        valid = sorted(rng.choice(g.nb, int(0.8 * g.nb), replace=False).tolist())
        bad = rng.choice(valid, int(0.2 * len(valid)), replace=False)
        blocks[bad, 4:] = rng.integers(-36, 37, (len(bad), 2))
        m = ref.fit_model(g, blocks, valid, ref.Fit())
        assert m is not None
        worst = max(worst, ref.corner_error(m[:4], truth, (g.H, g.W)))
    print('worst corner error', worst)
    assert worst < 0.3


def test_the_reachable_invalid_exits_of_the_case_file_are_what_they_claim():
    for name, n_valid in (('rotation_cap', None), ('zoom_cap', None), ('few_inliers', None), ('one_pair', 2), ('no_pair', 1)):
        g, out, _ = cases.want('invalid', name)
        assert not out['warp'][0, 1].any() and not out['inliers'][0, 1].any(), name
        assert out['shift'][0, 1, :3].tolist() == [0, 0, 0] and out['shift'][0, 1, 3] >= g.min_blocks, name
        if n_valid is not None:
            assert out['shift'][0, 1, 3] == n_valid, (name, out['shift'][0, 1].tolist())
        # the same scene under the default settings of the fit is valid where the exit is a setting's
        if name in ('rotation_cap', 'zoom_cap', 'few_inliers'):
            c = cases.case('invalid', name)
            again = ref.run([ref.Stream(g, ref.Fit())], cases.scene('invalid', name)[1])
            assert again['warp'][0, 1, 6] == 1, name


def test_small_reduction_cases_hold_a_valid_fit():
    """The GPU cases of every reduction are not all invalid frames: at least one frame per case reports a model -- but for
    k = 4, whose smallest shape has two blocks: there every frame leaves by the fewer-than-3-inliers exit."""
    for name in cases.REDUCTIONS:
        g, out, _ = cases.want('reduction', name)
        print(name, out['warp'][:, :, 6].tolist(), out['shift'][:, :, 3].tolist())
        if g.nb < 3:
            assert '-k4' in name and (out['shift'][:, 1:, 3] == 2).all() and not out['warp'].any(), name
        else:
            assert out['warp'][:, 1:, 6].any(), name


# ---- the tracker's predict step ----

def test_warp_predict_pure_shift_row_gives_the_shift_rule_bits():
    x = np.array([-0.0, 17.25, 10.0, 12.0, 179.5], np.float32)
    v = np.array([0.5, -0.25, 0.1, 0.0, 1.0], np.float32)
    nx, nv = ref.warp_predict(x, v, [0, 0, 0, 3 << 16, 65536, 0, 1, 9], (480, 640), 5)
    assert np.array_equal(nx.view(np.int32), (x + np.array([0, 3, 0, 0, 0], np.float32)).view(np.int32))
    assert np.array_equal(nv.view(np.int32), v.view(np.int32))
    # the skipped identity parts matter: (x + t) + (0 * ux - 0 * uy) turns a -0.0 into +0.0
    nx, _ = ref.warp_predict(np.array([-3.0, 0.0, 1.0, 1.0, 0.0], np.float32), v, [0, 0, 3 << 16, -0, 65536, 0, 1, 9], (480, 640), 5)
    assert nx[0] == 0.0 and not np.signbit(nx[0])                    # -3 + 3 = +0.0, as the shift rule gives it
    # a quarter-degree turn about the centre moves a box right of the centre down (y grows), and turns its angle forward
    row = [0, round(math.radians(0.25) * 65536), 0, 0, 65536, round(0.25 * 65536), 1, 9]
    nx, _ = ref.warp_predict(np.array([520.0, 240.0, 10.0, 12.0, 30.0], np.float32), v, row, (480, 640), 5)
    assert nx[1] > 240.0 and abs(nx[0] - 520.0) < 1e-3 and nx[4] == np.float32(30.25)


# ---- the bindings ----

def test_the_symbols_exist_and_the_abi_version_is_2():
    from mydetection_amd import _lib
    lib = _lib.lib()
    assert lib.mydet_abi_version() == 2
    for name in ('mydet_motion_warp_frames_rgb_u8', 'mydet_motion_warp_frames_yuv420', 'mydet_track_frames_warp_f32',
                 'mydet_track_frames_appear_warp_f32', 'mydet_track_frames_appear_optimal_warp_f32'):
        assert getattr(lib, name) is not None and name in _lib.SIGNATURES


def test_bad_values_are_errors_before_any_device_is_touched():
    import torch
    from mydetection_amd import ops
    from mydetection_amd.api import CameraMotion
    for kw in (dict(model='affine'), dict(model='similarity', max_zoom=0.3), dict(model='similarity', max_zoom=0),
               dict(model='similarity', max_rotation=15), dict(model='similarity', max_rotation=-1.0), dict(model='similarity', tolerance=0),
               dict(model='similarity', tolerance=17), dict(model='similarity', tolerance='2'), dict(model='shift', max_zoom=0.1),
               dict(max_rotation=3.0), dict(tolerance=1.0), dict(model='similarity', max_zoom=True)):
        with pytest.raises(ValueError):
            ops.motion_set(**kw)
        with pytest.raises(ValueError):
            CameraMotion(**kw)
    m = ops.motion_set(model='similarity', max_zoom=0.05, max_rotation=3.0, tolerance=1.5)
    assert list(m.reserved) == [1, 98304, 3277, 196608]
    assert list(ops.motion_set().reserved) == [0, 0, 0, 0] and list(ops.motion_set(model='similarity').reserved) == [1, 131072, 0, 0]
    cam = CameraMotion(model='similarity', max_rotation=3.0)
    assert repr(cam) == ("CameraMotion(reduce=None, search=8, min_texture=1024, min_blocks=None, model='similarity', max_zoom=None, "
                         'max_rotation=3.0, tolerance=2.0)')
    assert repr(CameraMotion()) == 'CameraMotion(reduce=None, search=8, min_texture=1024, min_blocks=None)'
    # shift= and warp= together: refused before anything else is looked at
    with pytest.raises(ValueError, match='shift and warp'):
        ops.track_frames(None, None, None, shift=torch.zeros(1, 1, 4, dtype=torch.int32), warp=torch.zeros(1, 1, 8, dtype=torch.int32))
    with pytest.raises(ValueError, match='inliers'):
        frames = torch.zeros(1, 96, 128, 3, dtype=torch.uint8)
        ops.motion_frames(frames, torch.zeros(1, ops.motion_geometry((96, 128), ops.motion_set())['state_words'], dtype=torch.int32),
                          ops.motion_set(), inliers=True)
