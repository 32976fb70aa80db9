"""CPU tests of the rotated-IoU NMS: the float64 checker (tests/_rotbox_ref.py) against the reference-made fixture
tests/golden/rot_iou.npz (tools/gen_rot_golden.py) and against crafted pairs with known IoU, and the argument errors and
defaults of the `rotated_nms` plumbing."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _rotbox_ref as chk  # noqa: E402


def crafted_pairs():
    """(name, box a, box b, expected IoU): duplicates, parallel and coincident edges, crossings, containment."""
    out = []
    for ang in (0.0, 30.0, 45.0, 90.0):
        out.append((f'identical at {ang:g}', [100, 120, 60, 30, ang], [100, 120, 60, 30, ang], 1.0))
    out += [
        ('the same box at +180', [100, 120, 60, 30, 17], [100, 120, 60, 30, 197], 1.0),
        ('w/h swapped at +90', [100, 120, 60, 30, 17], [100, 120, 30, 60, 107], 1.0),
        ('200x20 crossed at 45/135', [300, 300, 200, 20, 45], [300, 300, 200, 20, 135], 400.0 / 7600.0),
        ('axis-aligned half overlap', [100, 100, 40, 20, 0], [120, 100, 40, 20, 0], 1.0 / 3.0),
        ('disjoint', [100, 100, 40, 20, 0], [300, 100, 40, 20, 0], 0.0),
        ('edge touching', [100, 100, 40, 20, 0], [140, 100, 40, 20, 0], 0.0),
        ('contained', [100, 100, 40, 20, 30], [101, 99, 10, 6, 75], 60.0 / 800.0),
    ]
    return out


def thin_pairs():
    """Thin boxes (6 x 295 px, 49 : 1), where an angle error moves the long side most: duplicates, the same rectangle
    written with w and h swapped at +90 / +270, parallel-shifted copies, a crossing."""
    return [
        ('thin identical', [700, 400, 6, 295, 33], [700, 400, 6, 295, 33], 1.0),
        ('thin swapped at +90', [700, 400, 6, 295, 33], [700, 400, 295, 6, 123], 1.0),
        ('thin swapped at +270', [700, 400, 295, 6, -110.5], [700, 400, 6, 295, 159.5], 1.0),
        ('thin at +180', [700, 400, 6, 295, 171.25], [700, 400, 6, 295, 351.25], 1.0),
        ('thin shifted across by 2', [700, 400, 6, 295, 0], [702, 400, 6, 295, 0], 0.5),
        ('thin shifted along by 59', [700, 400, 6, 295, 90], [759, 400, 6, 295, 90], 236.0 / 354.0),
        ('thin crossed at right angles', [700, 400, 6, 295, 20], [700, 400, 6, 295, 110], 36.0 / (2 * 6 * 295 - 36)),
    ]


def duplicate_pairs(seed, n, thin):
    """n seeded pairs (a, b) of float32 boxes where b is a again, as the same rectangle -- unchanged, or turned by a
    multiple of 90 degrees with w and h swapped on the odd ones -- a third of them exactly (angles are multiples of 1/8
    degree, so the turned angle is exact in float32), a third with the centre moved by ~1e-3 px, a third with every field
    moved a little.  thin: 6-12 x 150-295 px (up to 49 : 1), else 5-350 px a side."""
    rng = np.random.Generator(np.random.PCG64(seed))
    a = np.empty((n, 5), np.float32)
    a[:, :2] = rng.uniform(50, 1500, (n, 2))
    if thin:
        a[:, 2] = rng.uniform(6, 12, n)
        a[:, 3] = rng.uniform(150, 295, n)
        sw = rng.random(n) < 0.5
        a[sw, 2], a[sw, 3] = a[sw, 3].copy(), a[sw, 2].copy()
    else:
        a[:, 2:4] = rng.uniform(5, 350, (n, 2))
    a[:, 4] = rng.integers(-2880, 2881, n) / 8.0
    b = a.copy()
    k = rng.integers(0, 4, n)
    odd = (k % 2) == 1
    b[odd, 2], b[odd, 3] = a[odd, 3], a[odd, 2]
    b[:, 4] = a[:, 4] + np.float32(90) * (k * rng.choice([-1, 1], n)).astype(np.float32)
    kind = np.arange(n) % 3
    b[kind == 1, :2] += rng.normal(0, 1e-3, ((kind == 1).sum(), 2)).astype(np.float32)
    m = kind == 2
    b[m] += (rng.normal(0, 1, (m.sum(), 5)) * [0.3, 0.3, 0.3, 0.3, 0.5]).astype(np.float32)
    return a, b, kind == 0


def test_checker_matches_the_reference_fixture(golden):
    g = golden('rot_iou')
    b = g['boxes']
    assert b.shape == (24, 5) and b.dtype == np.float32
    np.testing.assert_allclose(chk.vertices(b), g['ref_vertices'], rtol=0, atol=1e-4)
    mine = chk.iou_matrix(b, b)
    np.testing.assert_allclose(mine, g['exact_iou'], rtol=0, atol=1e-12)
    off = ~np.eye(24, dtype=bool)
    bound = float(g['mask_vs_exact_max'])
    assert np.abs(mine - g['mask_iou'])[off].max() <= bound + 1e-12
    # the fixture pins the angle convention: negated angles are off by more than ten times the discretisation error
    assert bound < float(g['flipped_angle_max']) / 10
    flipped = b.copy()
    flipped[:, 4] = -flipped[:, 4]
    assert np.abs(chk.iou_matrix(flipped, flipped) - g['mask_iou'])[off].max() > 10 * bound
    assert (mine[off] > 0.05).sum() > 100                  # the boxes overlap: the comparison is not about zeros


@pytest.mark.parametrize('name,a,b,want', crafted_pairs() + thin_pairs(), ids=[p[0] for p in crafted_pairs() + thin_pairs()])
def test_checker_on_crafted_pairs(name, a, b, want):
    assert abs(chk.iou_pairs([a], [b])[0] - want) <= 1e-12
    assert abs(chk.iou_pairs([b], [a])[0] - want) <= 1e-12


def test_checker_on_a_sweep_of_duplicates():
    """Coincident edges are where clipping can go wrong (a corner classified outside by round-off while its neighbours are
    inside makes the vertex list grow by more than one): every exact duplicate must come out as 1."""
    rng = np.random.Generator(np.random.PCG64(0))
    n = 50000
    x = np.concatenate([rng.uniform(0, 1500, (n, 2)), rng.uniform(2, 400, (n, 2)), rng.uniform(-360, 360, (n, 1))], 1).astype(np.float32)
    assert np.abs(chk.iou_pairs(x, x) - 1).max() <= 1e-9
    # the reviewer-style cases: two boxes for which a capped vertex list returned 1/3
    for a in ([234.88892, 810.4534, 338.66672, 265.32062, -55.435104], [1082.2076, 554.8906, 29.681957, 44.07503, -150.89903]):
        assert abs(chk.iou_pairs([a], [a])[0] - 1) <= 1e-9
    for thin in (False, True):
        a, b, exact = duplicate_pairs(1, 20000, thin)
        r = chk.iou_pairs(a, b)
        assert np.abs(r[exact] - 1).max() <= 1e-9, thin
        assert r.min() > 0.5, thin                           # the jittered ones stay near-duplicates
        np.testing.assert_allclose(chk.iou_pairs(b, a), r, rtol=0, atol=1e-9)
    # a box without area against a real one, rotated and partly overlapping: exactly 0, both ways round
    zero = np.array([[100, 100, 0, 60, 25]], np.float32)
    real = np.array([[110, 95, 40, 30, -40]], np.float32)
    assert chk.iou_pairs(zero, real)[0] == 0 and chk.iou_pairs(real, zero)[0] == 0


def test_checker_nms_order_and_rule():
    # three boxes of class 1 and one of class 0; box 2 duplicates box 0 (IoU 1) and scores lower
    boxes = np.array([[50, 50, 20, 10, 0], [200, 50, 20, 10, 30], [50, 50, 20, 10, 0], [50, 50, 20, 10, 0]], np.float32)
    cats = np.array([1, 1, 1, 0])
    scores = np.array([0.9, 0.9, 0.8, 0.1], np.float32)
    assert chk.nms(boxes, cats, scores, 0.05, 1.0).tolist() == [3, 0, 1]           # `>=`: IoU 1.0 at threshold 1.0 goes
    assert chk.nms(boxes, cats, scores, 0.05, 1.0, strict=True).tolist() == [3, 0, 1, 2]
    assert chk.nms(boxes, cats, scores, 0.5, 0.45).tolist() == [0, 1]
    zero = np.array([[5, 5, 0, 10, 0], [5, 5, 0, 10, 0]], np.float32)                # 0/0: not suppressed
    assert chk.nms(zero, np.zeros(2, np.int64), np.array([0.5, 0.4], np.float32), 0.1, 0.3).tolist() == [0, 1]


def test_rotated_nms_argument_errors():
    from mydetection_amd import ops
    from mydetection_amd.utils import bbox_ops
    from mydetection_amd.utils.structures import ImageObjects, batched_post_process
    b4 = torch.zeros(1, 3, 4)
    c, s = torch.zeros(1, 3, dtype=torch.int64), torch.ones(1, 3)
    with pytest.raises(ValueError):
        ops.postprocess(b4, c, s, 0.1, 0.5, rotated_nms=True)
    with pytest.raises(ValueError):
        ops.postprocess_dense(b4, c, s, 0.1, 0.5, rotated_nms=True)
    with pytest.raises(ValueError):
        batched_post_process(b4, c, s, 0.1, 0.5, rotated_nms=True)
    d = ImageObjects(b4[0], c[0], None, s[0])
    with pytest.raises(ValueError):
        d.post_process(0.1, 0.5, rotated_nms=True)
    with pytest.raises(ValueError):
        d.nms(0.5, rotated=True)
    with pytest.raises(ValueError):
        ImageObjects.non_max_suppression(d, 0.5, rotated=True)
    b5 = torch.zeros(3, 5)
    with pytest.raises(NotImplementedError):
        bbox_ops.nms_rotbb(b5, s[0], majority=3)
    with pytest.raises(NotImplementedError):
        bbox_ops.nms_rotbb(b5, s[0], bb_format='cxcywh')
    with pytest.raises(NotImplementedError):
        bbox_ops.nms_rotbb(torch.zeros(513, 5), torch.zeros(513))
    with pytest.raises(NotImplementedError):
        bbox_ops.iou_rotated(b5, b5, bb_format='x1y1x2y2')
    with pytest.raises(ValueError):
        bbox_ops.iou_rotated(b4[0], b5)
    keep = bbox_ops.nms_rotbb(torch.zeros(0, 5), torch.zeros(0))
    assert keep.dtype == torch.int64 and keep.shape == (0,)


def test_rotated_nms_is_opt_in():
    import inspect
    from mydetection_amd import configs, ops
    from mydetection_amd.graph import GraphedPath
    from mydetection_amd.utils.structures import ImageObjects, batched_post_process
    for name in configs.NAMES:
        assert 'test.rotated_nms' not in configs.get(name), name
    for fn, arg in ((ops.postprocess, 'rotated_nms'), (ops.postprocess_dense, 'rotated_nms'),
                    (batched_post_process, 'rotated_nms'), (ImageObjects.post_process, 'rotated_nms'),
                    (ImageObjects.nms, 'rotated'), (ImageObjects.non_max_suppression, 'rotated'),
                    (GraphedPath.__init__, 'rotated_nms')):
        assert inspect.signature(fn).parameters[arg].default is False, fn


def test_rotated_entry_points_check_arguments_before_launch():
    import ctypes
    from mydetection_amd import _lib
    lib = _lib.lib()
    null = ctypes.c_void_p(0)
    assert lib.mydet_postprocess_rotnms_f32(null, null, null, 1, 1 << 20, 0.5, 0.5, 512, null, null, null, null, null, null,
                                            null) == lib.mydet_postprocess_rot_f32(null, null, null, 1, 1 << 20, 0.5, 0.5, 512,
                                                                                   null, null, null, null, null, null, null)
    assert lib.mydet_postprocess_rotnms_f32(null, null, null, 1, 100, 0.5, 0.5, 513, null, null, null, null, null, null,
                                            null) == -1
    assert lib.mydet_postprocess_records_rotnms_f32(null, null, null, 1, 100, 0.5, 0.5, null, null, null) == -1
    assert lib.mydet_rotated_iou_f32(null, -1, null, 1, null, null) == -1
    assert lib.mydet_rotated_iou_f32(null, 0, null, 5, null, null) == 0
    assert lib.mydet_rotated_iou_f32(null, 2, null, 5, null, null) == -1
