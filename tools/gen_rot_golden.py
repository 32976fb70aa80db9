"""Writes tests/golden/rot_iou.npz: the rotated-IoU fixture (build container only -- it imports the reference).

24 seeded boxes of 40-220 px inside a 512^2 image; for them
  ref_vertices   the reference's xywha2vertex output (utils/bbox_ops.py:137-172), float32 [24,4,2]
  mask_iou       IoU of the reference's own rasterised masks, bbox_to_mask / vertex2masks at 512^2
                 (utils/bbox_ops.py:175-247), float64 [24,24]
  exact_iou      the float64 exact-area IoU of tests/_rotbox_ref.py, [24,24]
  mask_vs_exact_max, flipped_angle_max
                 largest |mask_iou - exact_iou|, and the same with every angle of the exact side negated (the wrong
                 convention): the first must be far below the second, which pins the vertex convention.
Only these arrays are stored; nothing of the reference's program text is.

    python tools/gen_rot_golden.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

SIZE = 512
N = 24


def boxes(seed=0):
    rng = np.random.Generator(np.random.PCG64(seed))
    b = np.empty((N, 5), np.float32)
    b[:, 2:4] = rng.uniform(40, 220, size=(N, 2))
    b[:, 0:2] = rng.uniform(170, SIZE - 170, size=(N, 2))          # half diagonal <= 156 px: every mask is inside
    b[:, 4] = rng.uniform(-180, 180, size=N)
    return b


def main():
    from oracle import _refimport
    _refimport.install()
    from utils import bbox_ops as ref
    import _rotbox_ref as chk

    b = boxes()
    t = torch.from_numpy(b)
    rad = t.clone()
    rad[:, 4] = rad[:, 4] / 180 * np.pi
    verts = ref.xywha2vertex(rad, is_degree=False).numpy()
    masks = ref.bbox_to_mask(t, bb_format='cxcywhd', mask_size=SIZE).numpy().astype(bool)
    assert masks.shape == (N, SIZE, SIZE)
    border = masks[:, 0].any() or masks[:, -1].any() or masks[:, :, 0].any() or masks[:, :, -1].any()
    assert not border, 'a mask touches the border'
    flat = masks.reshape(N, -1).astype(np.float64)
    inter = flat @ flat.T
    area = flat.sum(1)
    mask_iou = inter / (area[:, None] + area[None] - inter)
    exact = chk.iou_matrix(b, b)
    flipped = b.copy()
    flipped[:, 4] = -flipped[:, 4]
    off = ~np.eye(N, dtype=bool)
    mask_vs_exact = np.abs(mask_iou - exact)[off]
    flipped_max = np.abs(mask_iou - chk.iou_matrix(flipped, flipped))[off].max()
    print(f'pairs {off.sum() // 2}: |mask - exact| max {mask_vs_exact.max():.3e} mean {mask_vs_exact.mean():.3e}; '
          f'angles negated: max {flipped_max:.3e}')
    assert mask_vs_exact.max() < flipped_max / 10, 'the fixture does not pin the angle convention'
    np.testing.assert_allclose(chk.vertices(b), verts, rtol=0, atol=1e-4)
    out = os.path.join(ROOT, 'tests', 'golden', 'rot_iou.npz')
    np.savez_compressed(out, boxes=b, ref_vertices=verts.astype(np.float32), mask_iou=mask_iou, exact_iou=exact,
                        mask_vs_exact_max=np.float64(mask_vs_exact.max()), flipped_angle_max=np.float64(flipped_max),
                        mask_size=np.int64(SIZE))
    size = os.path.getsize(out)
    print(out, size, 'bytes')
    assert size < 16 * 1024


if __name__ == '__main__':
    main()
