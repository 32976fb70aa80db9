"""GPU tests of the Ultralytics (YOLOv5) decode: the kernel branch behind mydet_decode_uv5_levels_f32 against a float64
restatement and against DECODE_YOLO's scores, the multi-level launch against per-level launches, the reference layer's and
the reference ulo5m model's fixtures (tools/gen_golden_uv5.py), one decode launch per forward, hipGraph replay, Detector and
to_json."""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-4, 1e-4         # every candidate of a whole model, as the other model tests
# kernel against float64, the bounds tests/test_gpu_rapid.py::test_decode_rapid_vs_float64 uses for the YOLO-shaped columns.
# w = ((s*2) * (s*2)) * a squares the logistic, so its relative error is twice mydet_sigmoid's plus the roundings of the two
# products: mydet_sigmoid = 1 / (1 + expf(-x)) is off by at most ~2.5 ulp relative (expf 1 ulp, the sum and the correctly
# rounded quotient half an ulp each, the sum never cancels), 1.5e-7; twice that plus two half-ulp products is 3.6e-7, a fifth
# of the 2e-6 below: the bound needs no widening for this layer.
BOX_RTOL, BOX_ATOL, SCORE_RTOL, SCORE_ATOL = 2e-6, 1e-5, 2e-6, 1e-9

_spec = importlib.util.spec_from_file_location('uv5_host', os.path.join(os.path.dirname(__file__), 'test_uv5_host.py'))
_host = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_host)
uv5_f64 = _host.uv5_f64

ANCHORS = np.float32([[10, 13], [16, 30], [33, 23], [30, 61], [62, 45], [59, 119], [116, 90], [156, 198], [373, 326]])


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda')


def _head(B, A, H, W, C, ld, seed):
    """Pixel-major YOLO head rows [B,H,W,ld] (channel a*(5+C) + c: 4 box logits, objectness, C classes): class logits
    N(0, 2), a quarter of the box logits uniform in +-20; returns (tensor, t, conf, cls) with the raw views as numpy."""
    g = torch.Generator().manual_seed(seed)
    per = 5 + C
    x = torch.randn(B, H, W, ld, generator=g) * 2.0
    v = x[..., :A * per].view(B, H, W, A, per)
    wide = torch.rand(B, H, W, A, 4, generator=g) < 0.25
    v[..., :4] = torch.where(wide, torch.rand(B, H, W, A, 4, generator=g) * 40 - 20, v[..., :4] * 0.75)
    v[..., 4] -= 2.0
    t = v[..., :4].permute(0, 3, 1, 2, 4).numpy()
    conf = v[..., 4:5].permute(0, 3, 1, 2, 4).numpy()
    cls = v[..., 5:].permute(0, 3, 1, 2, 4).numpy()
    return x, t, conf, cls


def _outputs(dev, B, n, fill=None):
    if fill is None:
        return (torch.empty(B, n, 4, device=dev), torch.empty(B, n, dtype=torch.int64, device=dev), torch.empty(B, n, device=dev))
    return (torch.full((B, n, 4), float(fill), device=dev), torch.full((B, n), -1, dtype=torch.int64, device=dev),
            torch.full((B, n), float(fill), device=dev))


def _device_class_ids(cls, dev):
    """torch.max over the float32 logistic on the device: what the layer's class_idx is defined as."""
    return torch.sigmoid(torch.from_numpy(np.ascontiguousarray(cls)).to(dev)).max(-1).indices.reshape(cls.shape[0], -1).cpu().numpy()


# odd maps, padded pixel pitches, and batches of 3 whose 32-pixel tiles straddle images (H * W is not a multiple of 32)
@pytest.mark.parametrize('A,H,W,pad', [(3, 13, 11, 2), (1, 7, 9, 3)])
@pytest.mark.parametrize('C', [1, 15, 16, 80, 128])
def test_decode_uv5_vs_float64(dev, C, A, H, W, pad):
    from mydetection_amd import ops
    per = 5 + C
    ld = (A * per + 3) // 4 * 4 + 4 * (pad - 1)
    B, stride = 3, 16
    assert (H * W) % 32 and (2 * H * W) % 32
    x, t, conf, cls = _head(B, A, H, W, C, ld, seed=C * 100 + A * 10 + H)
    assert np.abs(t).max() > 19.5
    anchors = ANCHORS[3:3 + A]
    box = x.to(dev).permute(0, 3, 1, 2)                     # logical [B,ld,H,W], channels-last storage
    n = A * H * W
    out = _outputs(dev, B, n)
    ops.decode_uv5(box, ld, per, 0, box, ld, per, 5, 4, anchors, A, C, B, H, W, stride, (H * stride, W * stride), *out, 0)
    rb, ri, rs, gap = uv5_f64(t, conf, cls, anchors, stride)
    bb, ci, sc = (o.cpu().numpy() for o in out)
    print(f'C {C} A {A}: max rel box err {np.max(np.abs(bb - rb) / (np.abs(rb) + BOX_ATOL / BOX_RTOL)):.2e}, '
          f'max rel score err {np.max(np.abs(sc - rs) / rs):.2e}')
    np.testing.assert_allclose(bb, rb, rtol=BOX_RTOL, atol=BOX_ATOL)
    np.testing.assert_allclose(sc, rs, rtol=SCORE_RTOL, atol=SCORE_ATOL)
    # the ends of the parameterisation hold exactly and are reached
    a4 = 4 * np.tile(np.repeat(anchors, H * W, 0), (B, 1)).reshape(B, n, 2)
    assert (bb[..., 2:] <= a4).all() and (bb[..., 2:] >= 0).all() and (bb[..., :2] >= -stride / 2).all()
    assert (bb[..., 2:] == a4).sum() >= 1 and bb[..., 2:].min() < 1e-6
    lim = np.float32([(W + 0.5) * stride, (H + 0.5) * stride])
    assert (bb[..., :2] <= lim).all()
    if C > 1:
        safe = gap > 1e-6
        assert safe.mean() >= 0.99
        want = _device_class_ids(cls, dev)
        np.testing.assert_array_equal(ci[safe], want[safe])
        np.testing.assert_array_equal(ci[safe], ri[safe])
        assert len(np.unique(ci)) > 1
    else:
        assert not ci.any()


@pytest.mark.parametrize('C,A', [(1, 3), (16, 1), (80, 3), (128, 1)])
def test_scores_and_class_ids_equal_decode_yolo_bit_for_bit(dev, C, A):
    from mydetection_amd import ops
    B, H, W, stride = 3, 11, 13, 8
    per = 5 + C
    ld = (A * per + 3) // 4 * 4 + 4
    x, t, conf, cls = _head(B, A, H, W, C, ld, seed=7 + C)
    box = x.to(dev).permute(0, 3, 1, 2)
    n = A * H * W
    uv5, yolo = _outputs(dev, B, n), _outputs(dev, B, n)
    args = (box, ld, per, 0, box, ld, per, 5, 4, ANCHORS[:A], A, C, B, H, W, stride, (H * stride, W * stride))
    ops.decode_uv5(*args, *uv5, 0)
    ops.decode(ops.DECODE_YOLO, *args, *yolo, 0)
    assert torch.equal(uv5[1], yolo[1]) and torch.equal(uv5[2], yolo[2])
    assert not torch.equal(uv5[0], yolo[0])                 # ... and another box


def test_decode_uv5_levels_equal_per_level_launches(dev):
    from mydetection_amd import ops
    B, A, C = 2, 3, 80
    per = 5 + C
    ld = (A * per + 3) // 4 * 4
    shapes, strides = [(16, 12), (8, 6), (4, 3)], [8, 16, 32]
    heads = [_head(B, A, h, w, C, ld, seed=i)[0].to(dev).permute(0, 3, 1, 2) for i, (h, w) in enumerate(shapes)]
    anchors = ANCHORS.reshape(3, 3, 2)
    N = sum(A * h * w for h, w in shapes)
    one, per_level = _outputs(dev, B, N, np.nan), _outputs(dev, B, N, -7)
    levels, n_off = [], 0
    for i, ((h, w), hd) in enumerate(zip(shapes, heads)):
        levels.append(dict(box=hd, ldbox=ld, cls=hd, ldcls=ld, anchors_wh=anchors[i], H=h, W=w, stride=strides[i], n_off=n_off))
        ops.decode_uv5(hd, ld, per, 0, hd, ld, per, 5, 4, anchors[i], A, C, B, h, w, strides[i], (128, 96), *per_level, n_off)
        n_off += A * h * w
    ops.decode_uv5_levels(levels, per, 0, per, 5, 4, A, C, B, (128, 96), *one)
    for a, b in zip(one, per_level):
        assert torch.equal(a, b)
    assert not torch.isnan(one[0]).any() and int(one[1].min()) >= 0
    # a launch into the middle of larger arrays leaves the rest untouched
    part = _outputs(dev, B, N + 10, -7)
    lv = dict(levels[1], n_off=5)
    ops.decode_uv5_levels([lv], per, 0, per, 5, 4, A, C, B, (128, 96), *part)
    n1, o1 = A * 8 * 6, A * 16 * 12
    assert torch.equal(part[0][:, 5:5 + n1], one[0][:, o1:o1 + n1]) and torch.equal(part[2][:, 5:5 + n1], one[2][:, o1:o1 + n1])
    assert (part[0][:, :5] == -7).all() and (part[0][:, 5 + n1:] == -7).all() and (part[1][:, 5 + n1:] == -1).all()


def test_reference_layer_fixture_through_the_kernel(dev, golden):
    """uv5_layer.npz through DetectLayer.forward on a plain dict of raw views (the pack_pixel_major fallback)."""
    from mydetection_amd import configs
    from mydetection_amd.models.detlayers.uv5 import DetectLayer
    g = golden('uv5_layer')
    for n_cls in (1, 80):
        cfg = configs.get('ulo5m')
        cfg['model.fpn.out_strides'] = [int(s) for s in g['strides']] + [32]
        cfg['general.num_class'] = n_cls
        for lvl, (h, w) in enumerate(g['maps']):
            key = f'c{n_cls}_{h}x{w}'
            layer = DetectLayer(lvl, cfg)
            np.testing.assert_array_equal(layer.anchors.numpy(), g[f'{key}_anchors'])
            raw = {k: torch.from_numpy(g[f'{key}_{k}_in']).to(dev) for k in ('bbox', 'conf', 'class')}
            preds, loss = layer(raw, (h * layer.stride, w * layer.stride))
            assert loss is None and preds['bbox'].shape == (2, 3 * h * w, 4) and preds['class_idx'].dtype == torch.int64
            bb, ci, sc = (preds[k].cpu().numpy() for k in ('bbox', 'class_idx', 'score'))
            np.testing.assert_allclose(bb, g[f'{key}_bbox'], rtol=BOX_RTOL, atol=BOX_ATOL)
            np.testing.assert_allclose(sc, g[f'{key}_score'], rtol=SCORE_RTOL, atol=SCORE_ATOL)
            gap = uv5_f64(g[f'{key}_bbox_in'], g[f'{key}_conf_in'], g[f'{key}_class_in'], layer.anchors.numpy(), layer.stride)[3]
            safe = gap > 1e-6
            assert safe.mean() >= 0.99
            np.testing.assert_array_equal(ci[safe], g[f'{key}_class_idx'][safe])


def _model(dev, name):
    from mydetection_amd import synth
    from mydetection_amd.models.general import name_to_model
    m, cfg = name_to_model(name)
    m.load_state_dict(synth.make_state_dict(m.state_dict(), name), strict=True)
    return m.eval().to(dev), cfg


@pytest.fixture(scope='module')
def ulo5m(dev):
    return _model(dev, 'ulo5m')


@pytest.mark.parametrize('fixture', ['ulo5m_b1_256', 'ulo5m_b1_640'])
def test_model_vs_reference_fixture(dev, ulo5m, golden, fixture):
    """Every candidate within 1e-4, class ids exact where the reference's two best class probabilities are apart by more
    than float32 round-off, detections at the fixture's three settings: always the oracle's post-process of THESE
    candidates, and the reference's own (count, classes, order; scores and boxes 1e-4) wherever its decision margin exceeds
    twice the score error observed here.  Where the fixture holds every box, the post-process kernel on the REFERENCE's
    candidates reproduces the reference's detections and json rows exactly."""
    from mydetection_amd import synth
    from mydetection_amd.utils.structures import ImageObjects
    from oracle import postprocess as opp
    g = golden(fixture)
    m, cfg = ulo5m
    x = synth.make_images(1, int(g['size']), seed=int(g['image_seed'])).to(dev)
    with torch.no_grad():
        d = m(x)[0]
    n = g['scores_0'].shape[0]
    assert d.bboxes.shape == (n, 4) and d.cats.dtype == torch.int64 and d._bb_format == 'cxcywh'
    boxes, cats, scores = d.bboxes.cpu().numpy(), d.cats.cpu().numpy(), d.scores.cpu().numpy()
    err = float(np.abs(scores - g['scores_0']).max())
    print(f'{fixture}: max |score diff| {err:.2e}')
    np.testing.assert_allclose(scores, g['scores_0'], rtol=RTOL, atol=ATOL)
    ref = g['bboxes_0'] if 'bboxes_0' in g else g['bboxes_0_val']
    got = boxes if 'bboxes_0' in g else boxes[g['bboxes_0_idx']]
    np.testing.assert_allclose(got, ref, rtol=RTOL, atol=ATOL)
    safe = g['cls_margin_0'] > 2e-5
    assert safe.mean() > 0.99, 'fixture has too many tied classes'
    np.testing.assert_array_equal(cats[safe], g['cats_0'][safe])
    assert len(np.unique(cats)) > 10
    for tag in ('ap', 'mid', 'demo'):
        conf, nms = float(g[f'pp_{tag}_conf']), float(g[f'pp_{tag}_nms'])
        r = d.post_process(conf, nms)
        ob, oc, os_, _ = opp.post_process(boxes, cats, scores, conf, nms)
        np.testing.assert_array_equal(r.cats.cpu().numpy(), oc, err_msg=f'{fixture} {tag}')
        np.testing.assert_array_equal(r.scores.cpu().numpy(), os_, err_msg=f'{fixture} {tag}')
        np.testing.assert_array_equal(r.bboxes.cpu().numpy().reshape(-1, 4), ob.reshape(-1, 4), err_msg=f'{fixture} {tag}')
        ref_c, ref_s, ref_b = g[f'pp_{tag}_cats_0'], g[f'pp_{tag}_scores_0'], g[f'pp_{tag}_bboxes_0']
        margin = float(g[f'pp_{tag}_margin'])
        print(f'{fixture} {tag}: {len(r)} detections, reference {len(ref_c)}, margin {margin:.1e}')
        if margin > 2 * err:
            assert len(r) == len(ref_c) and np.array_equal(r.cats.cpu().numpy(), ref_c), f'{fixture} {tag}'
            np.testing.assert_allclose(r.scores.cpu().numpy(), ref_s, rtol=RTOL, atol=ATOL)
            np.testing.assert_allclose(r.bboxes.cpu().numpy().reshape(-1, 4), ref_b, rtol=RTOL, atol=ATOL)
        if 'bboxes_0' in g and margin > 0.0:        # (exact score ties are broken by torch.topk's unspecified order)
            ref_d = ImageObjects(torch.from_numpy(g['bboxes_0']).to(dev), torch.from_numpy(g['cats_0']).to(dev), None,
                                 torch.from_numpy(g['scores_0']).to(dev), 'cxcywh', d.img_hw)
            rr = ref_d.post_process(conf, nms)
            np.testing.assert_array_equal(rr.cats.cpu().numpy(), ref_c, err_msg=f'{fixture} {tag}')
            np.testing.assert_array_equal(rr.scores.cpu().numpy(), ref_s, err_msg=f'{fixture} {tag}')
            np.testing.assert_array_equal(rr.bboxes.cpu().numpy().reshape(-1, 4), ref_b, err_msg=f'{fixture} {tag}')
            assert rr.to_json(7) == json.loads(str(g[f'pp_{tag}_json_0'])), f'{fixture} {tag}'
    assert len(g['pp_ap_cats_0']) > 100


@pytest.mark.parametrize('size,seed', [(256, 4), (320, 2)])
def test_scores_and_class_ids_equal_u5m_yv3(dev, ulo5m, size, seed):
    """The same weights and image under the two decoders: scores and class ids bit for bit, boxes not."""
    from mydetection_amd import synth
    m, _ = ulo5m
    y, _ = _model(dev, 'u5m_yv3')
    x = synth.make_images(2, size, seed=seed).to(dev)
    with torch.no_grad():
        a, b = m.forward_candidates(x), y.forward_candidates(x)
    assert a[0].shape == b[0].shape == (2, 3 * 21 * (size // 32) ** 2, 4)
    assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    assert not torch.equal(a[0], b[0])
    # the same cell and the same logit: the centres differ by (sigmoid - 0.5) * stride, at most half the coarsest stride
    assert float((a[0][..., :2] - b[0][..., :2]).abs().max()) <= 0.5 * 32 + 1e-3


def test_one_decode_launch_per_forward(dev, ulo5m):
    from mydetection_amd import ops, synth
    m, _ = ulo5m
    x = synth.make_images(2, 256, seed=5).to(dev)
    with torch.no_grad():
        want = m.forward_candidates(x)
        ops.TIMER = ops.KernelTimer()
        try:
            got = m.forward_candidates(x)
        finally:
            timer, ops.TIMER = ops.TIMER, None
        torch.cuda.synchronize()
        assert len(timer.spans.get('decode', [])) == 1
        for a, b in zip(got, want):
            assert torch.equal(a, b)
        # a lone layer on its own level's raw predictions agrees with its slice of the single launch
        raws = m.rpn(m.fpn(m.backbone(x)))
        n_off = 0
        for layer, raw in zip(m.det_layers, raws):
            preds, _ = layer(raw, x.shape[2:4])
            k = preds['score'].shape[1]
            assert torch.equal(preds['bbox'], want[0][:, n_off:n_off + k])
            assert torch.equal(preds['class_idx'], want[1][:, n_off:n_off + k])
            assert torch.equal(preds['score'], want[2][:, n_off:n_off + k])
            n_off += k
        assert n_off == want[2].shape[1]


def test_graph_replay_equals_eager(dev, ulo5m):
    from mydetection_amd import synth
    from mydetection_amd.graph import GraphedPath
    m, cfg = ulo5m
    x = torch.cat([synth.make_images(1, 256, seed=s) for s in range(4)]).to(dev)
    gp = GraphedPath(m, x, 0.005, cfg['test.nms_thres'], lanes=1)
    rec = {k: v.clone() for k, v in gp(x).items()}
    eager = gp.eager(x)
    assert 'angle' not in rec
    for k in ('count', 'bbox', 'score', 'class_idx', 'index'):
        assert torch.equal(rec[k], eager[k]), k
    assert int(rec['count'].min()) > 0
    x2 = x.flip(0).contiguous()
    rec2 = gp(x2)
    for k in ('count', 'bbox', 'score', 'class_idx', 'index'):
        assert torch.equal(rec2[k], gp.eager(x2)[k]), k


def test_detector_predict_batch_and_json(dev):
    import PIL.Image
    from mydetection_amd import synth
    from mydetection_amd.api import Detector
    from mydetection_amd.utils.structures import batched_to_json
    det = Detector(model_name='ulo5m')
    det.model.load_state_dict(synth.make_state_dict(det.model.state_dict(), 'ulo5m'), strict=True)
    assert det.input_size == 640 and det.conf_thres == 0.5 and det.nms_thres == 0.45 and det.divisibe == 32
    imgs = []
    # one image per network input size, so that predict_batch's forward sees the same batch as detect_one's (a solo image
    # and the same image inside a batch differ in the last float bits) and the comparison can be bit for bit
    for i, (h, w) in enumerate([(300, 400), (250, 380), (400, 230), (256, 256)]):
        arr = (synth.make_images(1, max(h, w), seed=20 + i)[0, :, :h, :w].permute(1, 2, 0).numpy() * 255).astype(np.uint8)
        imgs.append(PIL.Image.fromarray(arr))
    kw = dict(input_size=320, conf_thres=0.05)
    batch = det.predict_batch(imgs, **kw)
    assert len(batch) == 4
    total = 0
    for img, got in zip(imgs, batch):
        one = det.detect_one(pil_img=img, **kw)
        assert got.bboxes.shape[1] == 4 and got.img_hw == (img.height, img.width)
        assert torch.equal(got.bboxes, one.bboxes) and torch.equal(got.scores, one.scores) and torch.equal(got.cats, one.cats)
        total += len(got)
    assert total > 0
    for idxs, rec in det._records_by_size(imgs, **kw):
        rows = batched_to_json(rec, [f'im{j}' for j in idxs])
        want = [r for j in idxs for r in batch[j].to_json(f'im{j}')]
        assert rows == want
        json.dumps(rows)
