"""GPU tests of the similarity model of the camera-motion estimator (include/mydet.h: mydet_motion_warp_frames_rgb_u8 / _yuv420;
csrc/motion.hip: the refine stage around each block's own vector, motion_fit_kernel).

The checker is tests/_warp_ref.py, the rule text in Python integers, which tests/test_warp_host.py holds to known transforms.
Everything is integer arithmetic: out_warp, out_shift, out_blocks, the inlier mask and every field of the state equal the
restatement with ==.  The cases and what the restatement makes of them come from tests/_warp_cases.py, computed once."""
import numpy as np
import pytest
import torch

import _motion_ref as mref
import _warp_cases as cases
from test_gpu_motion import _assert_motion_state, _planes

pytestmark = pytest.mark.gpu

FILL = -77


def _images(c, y8):
    """image_of(f0, n) and the layout for the frames y8 uint8 [S, F, H, W] of a case, on the device."""
    S = y8.shape[0]
    if c['source'] == 'rgb':
        rgb = np.repeat(y8[..., None], 3, axis=-1)
        return (lambda f0, n: torch.from_numpy(np.ascontiguousarray(rgb[:, f0:f0 + n]).reshape((S * n,) + rgb.shape[2:])).cuda()), None
    F = y8.shape[1]
    planes, stored = _planes(c['source'], y8.reshape((S * F,) + y8.shape[2:]), 4, seed=11)
    assert np.array_equal(mref.luma_y(stored, c['source']), y8.reshape(stored.shape))

    def image_of(f0, n):
        idx = torch.tensor([s * F + f for s in range(S) for f in range(f0, f0 + n)]).cuda()
        return [p.index_select(0, idx) for p in planes]
    return image_of, c['source']


def _run(group, name, splits=None):
    """The kernels on a case, in one call or in the calls `splits` names, against the restatement's one call; the outputs are
    passed in filled, so that what the kernels leave unwritten shows."""
    from mydetection_amd import ops
    c = cases.case(group, name)
    g, want, streams = cases.want(group, name)
    y8, _ = cases.scene(group, name)
    S, F = y8.shape[:2]
    image_of, layout = _images(c, y8)
    mset = ops.motion_set(model='similarity', **c['set'])
    state = ops.motion_state(S, c['hw'], mset, 'cuda')
    parts, lo = [], 0
    for n in splits or [F]:
        out = {k: torch.full((S, n) + shape, FILL, dtype=torch.int32, device='cuda')
               for k, shape in (('shift', (4,)), ('warp', (8,)), ('blocks', (g.nb, 6)), ('inliers', (g.nb,)))}
        parts.append(ops.motion_frames(image_of(lo, n), state, mset, frames_per_stream=n, layout=layout, out=out, inliers=True))
        lo += n
    assert lo == F
    got = {k: torch.cat([p[k] for p in parts], dim=1).cpu().numpy() for k in ('shift', 'warp', 'blocks', 'inliers')}
    for k in ('blocks', 'shift', 'warp', 'inliers'):
        assert got[k].dtype == np.int32 and got[k].shape == want[k].shape, k
        assert np.array_equal(got[k], want[k]), (k, np.argwhere(got[k] != want[k])[:8].tolist(), got['warp'].tolist(), want['warp'].tolist())
    _assert_motion_state(state, c['hw'], mset, streams)
    return want, state, mset


@pytest.mark.parametrize('name', sorted(cases.REDUCTIONS))
def test_every_reduction_and_source_equals_the_restatement(name):
    """k = 2, 4, 8 at their smallest odd shapes, RGB, NV12 and P010, one and two streams of three frames."""
    _run('reduction', name)


@pytest.mark.parametrize('name', sorted(cases.SCENES))
def test_a_real_fit_equals_the_restatement(name):
    """320 x 448 (117 blocks) and 262 x 382 (15 blocks): turns, zooms and a pure shift, each a valid fit."""
    want, *_ = _run('scene', name)
    assert want['warp'][0, 1, 6] == 1
    if name == 'pure_shift':
        assert want['warp'][0, 1].tolist() == [0, 0, 7 << 16, -9 << 16, 65536, 0, 1, 117]


def test_foreign_blocks_equal_the_restatement():
    want, *_ = _run('outliers', 'quarter')
    assert want['warp'][0, 1, 6] == 1 and 0 < want['warp'][0, 1, 7] < want['shift'][0, 1, 3]


def test_more_blocks_than_threads():
    """560 x 528, k = 2, R = 4: 272 blocks, so the fit's loops over blocks and pairs take a second pass."""
    want, *_ = _run('many', '272')
    assert want['shift'][0, 1, 3] > 256 and want['warp'][0, 1, 6] == 1


def test_a_split_call_equals_one_call():
    _run('split', 'split', splits=[1, 2])


@pytest.mark.parametrize('name', sorted(cases.INVALID))
def test_every_reachable_invalid_exit(name):
    """A cap exceeded, fewer than three inliers with many blocks, one pair, no pair: zero rows, valid 0, n_valid kept."""
    want, *_ = _run('invalid', name)
    assert not want['warp'][0, 1].any() and want['shift'][0, 1, :3].tolist() == [0, 0, 0] and want['shift'][0, 1, 3] >= 1


def test_flat_frames_and_a_scene_cut_report_no_motion():
    from mydetection_amd import ops
    hw = (96, 128)
    mset = ops.motion_set(model='similarity', reduce=2, search=8)
    g = mref.Geometry(hw, 2, 8)
    flat = torch.full((3,) + hw + (3,), 90, dtype=torch.uint8, device='cuda')
    out = ops.motion_frames(flat, ops.motion_state(1, hw, mset, 'cuda'), mset, inliers=True)
    assert not out['warp'].any() and not out['shift'].any() and not out['inliers'].any() and not out['blocks'][..., 4:].any()
    tex_a, tex_b = mref.coarse_texture(200, 230, 1), mref.coarse_texture(200, 230, 2)
    cut = np.stack([tex_a[40:136, 40:168], tex_a[42:138, 37:165], tex_b[40:136, 40:168], tex_b[39:135, 44:172]])
    lumas = cut.astype(np.int64)[None]
    import _warp_ref as ref
    streams = [ref.Stream(g, ref.Fit())]
    want = ref.run(streams, lumas)
    state = ops.motion_state(1, hw, mset, 'cuda')
    got = ops.motion_frames(torch.from_numpy(np.repeat(cut[..., None], 3, axis=-1)).cuda(), state, mset, inliers=True)
    for k in want:
        assert np.array_equal(got[k].cpu().numpy(), want[k]), k
    assert want['shift'][0, :, :3].tolist() == [[0, 0, 0], [3, -2, 1], [0, 0, 0], [-4, 1, 1]] and not want['warp'][0, 2].any()
    _assert_motion_state(state, hw, mset, streams)


def test_the_shift_mode_entry_points_give_what_they_gave():
    """The same frames through a set of model 'shift': the outputs and the state of tests/_motion_ref.py, no 'warp' key; and a
    state written by one family continues in the other (one layout)."""
    from mydetection_amd import ops
    c = cases.case('scene', 'turn_k4')
    y8, lumas = cases.scene('scene', 'turn_k4')
    g = cases.geometry(c)
    streams = [mref.Stream(g)]
    want_shift, want_blocks = mref.run(streams, lumas)
    image_of, _ = _images(c, y8)
    mset = ops.motion_set(**c['set'])
    state = ops.motion_state(1, c['hw'], mset, 'cuda')
    got = ops.motion_frames(image_of(0, 2), state, mset)
    assert sorted(got) == ['blocks', 'shift']
    assert np.array_equal(got['shift'].cpu().numpy(), want_shift) and np.array_equal(got['blocks'].cpu().numpy(), want_blocks)
    _assert_motion_state(state, c['hw'], mset, streams)
    # frame 1 again, against the state the shift family left: the similarity family reads the same layout
    wset = ops.motion_set(model='similarity', **c['set'])
    again = ops.motion_frames(image_of(1, 1), state, wset)
    assert again['warp'][0, 0].tolist() == [0, 0, 0, 0, 65536, 0, 1, g.nb] and again['shift'][0, 0].tolist() == [0, 0, 1, g.nb]
