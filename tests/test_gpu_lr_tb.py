"""GPU tests of the lr_tb box head (mydet_lr_tb_levels_f32, _LR_TB_last, configs d1_fcs2s / d1_fcs2s_mos): the kernel
against a float64 restatement, the multi-level launch against per-level launches, the whole model against the fixtures
made from the imported reference (tools/gen_golden_lr_tb.py), graph replay and batch lanes."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def _load(name):
    """A sibling test module's helpers, loaded from its file (whatever pytest's import mode)."""
    spec = importlib.util.spec_from_file_location('_lr_tb_' + name, os.path.join(HERE, name + '.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


_host = _load('test_lr_tb_host')
layer_weights, lr_tb_f64 = _host.layer_weights, _host.lr_tb_f64


def _gpu_model_tests():
    return _load('test_gpu_model')


def _packed(C, seed):
    from mydetection_amd import ops
    g = torch.Generator().manual_seed(seed)
    ws = [torch.randn(C, 1, 3, 3, generator=g), torch.randn(C, 1, 3, 3, generator=g), torch.randn(2, C, 1, 3, generator=g) * 0.3,
          torch.randn(2, generator=g), torch.randn(2, C, 3, 1, generator=g) * 0.3, torch.randn(2, generator=g)]
    lr0, tb0, lr1, blr, tb1, btb = ws
    return ws, ops.pack_lr_tb(lr0, tb0, lr1, blr, tb1, btb).cuda()


def _ref(x, ws):
    lr0, tb0, lr1, blr, tb1, btb = ws
    return lr_tb_f64(x.cpu().numpy(), lr0, lr1, blr, tb0, tb1, btb).numpy()


def _close(y, ref, what):
    err = float(np.abs(y.astype(np.float64) - ref).max())
    rms = float(np.sqrt((ref ** 2).mean()))
    assert err <= 1e-5 * rms, f'{what}: max error {err:.2e} vs rms {rms:.2e}'


def test_kernel_vs_float64_on_the_reference_layer_fixture(golden):
    from mydetection_amd import ops, synth
    g = golden('lr_tb_layer')
    B, C = int(g['B']), int(g['C'])
    lr0, lr1, blr, tb0, tb1, btb = (torch.from_numpy(np.asarray(a)) for a in layer_weights(g))
    w = ops.pack_lr_tb(lr0, tb0, lr1, blr, tb1, btb).cuda()
    xs = [torch.from_numpy(g[f'x_{h}x{wd}'] if f'x_{h}x{wd}' in g else synth._normal(f'lr_tb_layer.x{h}x{wd}', (B, C, h, wd)))
          for h, wd in g['maps']]
    outs = ops.lr_tb_levels([(x.cuda(), w) for x in xs])           # all six maps in one launch
    torch.cuda.synchronize()
    for (h, wd), x, y in zip(g['maps'], xs, outs):
        assert tuple(y.shape) == (B, 4, h, wd) and ops.nhwc_ld(y) == 4
        ref = lr_tb_f64(x.numpy(), *layer_weights(g)).numpy()
        _close(y.cpu().numpy(), ref, f'{h}x{wd}')
        if f'y_{h}x{wd}' in g:                                   # and the reference's own float32 output
            np.testing.assert_allclose(y.cpu().numpy(), g[f'y_{h}x{wd}'], rtol=1e-5, atol=1e-5)


def _raw_launch(xs, ldx, w, C, offset=0):
    """The C ABI directly: maps stored [B,H,W,ldx] (any ldx >= C) starting `offset` floats into their buffers."""
    from mydetection_amd import _lib, ops
    arr = (_lib.LrTbLevel * len(xs))()
    keep, outs = [], []
    for i, x in enumerate(xs):
        B, _, H, W = x.shape
        buf = torch.zeros(offset + B * H * W * ldx, device='cuda')
        buf[offset:].view(B, H, W, ldx)[..., :C] = x.permute(0, 2, 3, 1).cuda()
        y = torch.full((B, H, W, 4), float('nan'), device='cuda')
        arr[i] = _lib.LrTbLevel(buf.data_ptr() + 4 * offset, ldx, w.data_ptr(), y.data_ptr(), 4, H, W)
        keep.append(buf)
        outs.append(y)
    _lib.check(_lib.lib().mydet_lr_tb_levels_f32(len(xs), ctypes.cast(arr, ctypes.c_void_p), xs[0].shape[0], C, ops._stream()),
               'mydet_lr_tb_levels_f32')
    torch.cuda.synchronize()
    return [y.permute(0, 3, 1, 2).cpu().numpy() for y in outs]


@pytest.mark.parametrize('B,C,ldx,offset', [(1, 88, 88, 0), (3, 88, 96, 0), (3, 40, 40, 0), (1, 88, 90, 1), (2, 128, 128, 0)])
def test_kernel_on_random_level_tables(B, C, ldx, offset):
    """Five non-square levels (40x24 ... 3x2) in one launch: batch 1 / 3, C 88 / 40 / 128 (past 64 KiB of LDS), a pitch
    larger than C, and a pitch that is not a multiple of 4 floats at an unaligned base (the scalar-load path)."""
    ws, w = _packed(C, seed=C + ldx)
    g = torch.Generator().manual_seed(B * 1000 + ldx)
    xs = [torch.randn(B, C, h, wd, generator=g) for h, wd in ((40, 24), (20, 12), (10, 6), (5, 3), (3, 2))]
    for x, y in zip(xs, _raw_launch(xs, ldx, w, C, offset)):
        _close(y, _ref(x, ws), f'{tuple(x.shape)} ldx {ldx}')


def test_multi_level_launch_equals_per_level_launches():
    from mydetection_amd import ops
    ws, w = _packed(88, seed=3)
    g = torch.Generator().manual_seed(9)
    xs = [torch.randn(2, 88, h, h, generator=g).cuda() for h in (80, 40, 20, 10, 5)]
    ws2, w2 = _packed(88, seed=4)                                # levels with different weights, as in the head
    levels = [(x, w if i % 2 else w2) for i, x in enumerate(xs)]
    together = ops.lr_tb_levels(levels)
    alone = [ops.lr_tb_levels([lv])[0] for lv in levels]
    torch.cuda.synchronize()
    for a, b in zip(together, alone):
        assert torch.equal(a, b)


@pytest.fixture(scope='module')
def fcs2s():
    from mydetection_amd import synth
    from mydetection_amd.models.general import name_to_model
    m, cfg = name_to_model('d1_fcs2s')
    m.load_state_dict(synth.make_state_dict(m.state_dict(), 'd1_fcs2s'), strict=True)
    return m.eval().cuda(), cfg


@pytest.mark.parametrize('fixture', ['d1_fcs2s_b1_256', 'd1_fcs2s_b1_640'])
def test_d1_fcs2s_vs_reference_golden(fcs2s, golden, fixture):
    """Stage samples, head logits ('bbox' included), all candidates within 1e-4, class ids where defined, detections at
    three settings: the checks of tests/test_gpu_model.py::_check_effdet_golden."""
    m, _ = fcs2s
    _gpu_model_tests()._check_effdet_golden(fixture, m, golden(fixture))


def test_box_layers_are_one_launch_and_a_lone_layer_agrees(fcs2s):
    from mydetection_amd import ops, synth
    from mydetection_amd.models.rpns import _LR_TB_last
    m, _ = fcs2s
    x = synth.make_normalized_images(2, 256, seed=5).cuda()
    with torch.no_grad():
        p = m.fpn(m.backbone(x))
        ops.TIMER = ops.KernelTimer()
        try:
            raws = m.rpn(p)
        finally:
            timer, ops.TIMER = ops.TIMER, None
        torch.cuda.synchronize()
        assert len(timer.spans.get('lr_tb', [])) == 1
        _, box_t = m.rpn._tower_layers(p)
        for i, t in enumerate(box_t):
            last = m.rpn.bbox_nets[i][3]
            assert isinstance(last, _LR_TB_last)
            assert torch.equal(last(t).permute(0, 2, 3, 1), raws[i]['bbox'])
        # an in-place edit of a weight is seen (the versioned cache of the packed weights)
        before = m.rpn.bbox_nets[4][3](box_t[4]).clone()
        m.rpn.bbox_nets[4][3]._tb[1].bias.add_(1.0)
        after = m.rpn.bbox_nets[4][3](box_t[4])
        m.rpn.bbox_nets[4][3]._tb[1].bias.sub_(1.0)
        torch.testing.assert_close(after[:, 1::2] - before[:, 1::2], torch.ones_like(after[:, 1::2]), rtol=0, atol=1e-5)
        assert torch.equal(after[:, 0::2], before[:, 0::2])


def test_hipgraph_replay_equals_eager(fcs2s):
    from mydetection_amd import synth
    from mydetection_amd.graph import GraphedPath
    from mydetection_amd.utils.structures import batched_post_process
    m, _ = fcs2s
    x0 = synth.make_normalized_images(2, 256, seed=21).cuda()
    x1 = synth.make_normalized_images(2, 256, seed=22).cuda()
    run = GraphedPath(m, x0, 0.005, 0.45, lanes=1)
    for x in (x0, x1, x0):
        rec = {k: v.clone() for k, v in run(x).items()}
        with torch.no_grad():
            ref = batched_post_process(*m.forward_candidates(x), 0.005, 0.45)
        assert int(ref['count'].sum()) > 0
        for k in ('count', 'index', 'class_idx', 'score', 'bbox'):
            assert torch.equal(rec[k], ref[k]), k


def test_detector_predict_batch_lanes_vs_detect_one(fcs2s, monkeypatch):
    import PIL.Image
    from mydetection_amd import synth
    from mydetection_amd.api import Detector
    monkeypatch.delenv('MYDET_LANES', raising=False)
    m, cfg = fcs2s
    det = Detector(model_and_cfg=(m, cfg))
    assert det.batch_lanes(4) == 2
    imgs = [PIL.Image.fromarray((synth.make_images(1, (256, 256), seed=70 + i)[0].permute(1, 2, 0).numpy() * 255).astype(np.uint8))
            for i in range(4)]
    kw = dict(preprocessing='resize_pad_square', input_size=256, conf_thres=0.05)
    batched = det.predict_batch(imgs, **kw)
    assert sum(len(d) for d in batched) > 0
    for img, d in zip(imgs, batched):
        e = det.detect_one(pil_img=img, **kw)
        assert len(d) == len(e)
        assert torch.equal(d.cats.cpu(), e.cats.cpu())
        np.testing.assert_allclose(d.bboxes.cpu().numpy(), e.bboxes.cpu().numpy(), rtol=1e-4, atol=1e-4)
        np.testing.assert_allclose(d.scores.cpu().numpy(), e.scores.cpu().numpy(), rtol=1e-4, atol=1e-4)
