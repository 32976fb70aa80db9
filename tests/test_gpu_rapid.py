"""GPU tests of the RAPiD rotated-box path: the DECODE_RAPID mode of the decode kernel against a float64 restatement, the
multi-level launch against per-level launches, the rotated post-process against the 4-column one, the five RAPiD configs
against the imported reference's fixtures (tools/gen_golden_rapid.py), hipGraph replay, Detector and to_json('cxcywhd')."""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-4, 1e-4         # boxes (columns 0-3) and scores, as the other model tests
ANGLE_ATOL = 2e-2               # degrees: d deg / d logit <= 90, so a head logit off by 1e-4 moves the angle by <= 9e-3

_spec = importlib.util.spec_from_file_location('rapid_host', os.path.join(os.path.dirname(__file__), 'test_rapid_host.py'))
_host = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_host)
rapid_f64 = _host.rapid_f64


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda')


def _head(B, A, H, W, C, ld, seed):
    """Pixel-major head rows [B,H,W,ld] (channel a*(6+C) + c), angle logits out to +-17; returns (tensor, t, conf, cls)."""
    g = torch.Generator().manual_seed(seed)
    per = 6 + C
    x = torch.randn(B, H, W, ld, generator=g) * 2.0
    v = x[..., :A * per].view(B, H, W, A, per)
    v[..., 4] = torch.rand(B, H, W, A, generator=g) * 34 - 17
    v[..., 5] -= 2.0
    t = v[..., :5].permute(0, 3, 1, 2, 4).numpy()
    conf = v[..., 5:6].permute(0, 3, 1, 2, 4).numpy()
    cls = v[..., 6:].permute(0, 3, 1, 2, 4).numpy()
    return x, t, conf, cls


@pytest.mark.parametrize('C,A,H,W,pad', [(0, 3, 13, 11, 2), (0, 1, 7, 9, 2), (1, 3, 5, 17, 3), (80, 3, 9, 7, 2),
                                         (80, 1, 11, 5, 6), (1, 1, 3, 3, 1)])
def test_decode_rapid_vs_float64(dev, C, A, H, W, pad):
    from mydetection_amd import ops
    per = 6 + C
    ld = (A * per + 3) // 4 * 4 + 4 * (pad - 1)             # padded pixel pitches
    B, stride = 2, 16
    x, t, conf, cls = _head(B, A, H, W, C, ld, seed=C * 100 + A * 10 + H)
    anchors = np.float32([[18.7807, 33.4659], [28.8912, 61.7536], [48.6849, 68.3897]][:A])
    box = x.to(dev).permute(0, 3, 1, 2)                     # logical [B,ld,H,W], channels-last storage
    n = A * H * W
    out = (torch.empty(B, n, 5, device=dev), torch.empty(B, n, dtype=torch.int64, device=dev), torch.empty(B, n, device=dev))
    ops.decode(ops.DECODE_RAPID, box, ld, per, 0, box, ld, per, 6, 5, anchors, A, C, B, H, W, stride, (H * stride, W * stride),
               *out, 0)
    rb, ri, rs = rapid_f64(t, conf, cls, anchors, stride)
    bb, ci, sc = (o.cpu().numpy() for o in out)
    np.testing.assert_allclose(bb[..., :4], rb[..., :4], rtol=2e-6, atol=1e-5)
    np.testing.assert_allclose(bb[..., 4], rb[..., 4], rtol=0, atol=1e-4)
    np.testing.assert_allclose(sc, rs, rtol=2e-6, atol=1e-9)
    assert np.abs(bb[..., 4]).max() <= 180.0 and np.abs(bb[..., 4]).max() > 179.99
    if C > 1:
        p = np.sort(1 / (1 + np.exp(-cls.astype(np.float64))), -1).reshape(B, -1, C)
        safe = p[..., -1] - p[..., -2] > 1e-6
        np.testing.assert_array_equal(ci[safe], ri[safe])
    else:
        assert not ci.any()


def test_decode_rapid_levels_equal_per_level_launches(dev):
    from mydetection_amd import ops
    B, A, C = 2, 3, 80
    per = 6 + C
    ld = (A * per + 3) // 4 * 4
    shapes, strides = [(16, 12), (8, 6), (4, 3)], [8, 16, 32]
    heads = [_head(B, A, h, w, C, ld, seed=i)[0].to(dev).permute(0, 3, 1, 2) for i, (h, w) in enumerate(shapes)]
    anchors = np.float32([[18.8, 33.5], [28.9, 61.8], [48.7, 68.4], [45.1, 101.5], [63.1, 113.5], [81.4, 134.5],
                          [91.7, 145.0], [137.5, 178.5], [194.4, 250.8]]).reshape(3, 3, 2)
    N = sum(A * h * w for h, w in shapes)
    one = (torch.full((B, N, 5), np.nan, device=dev), torch.full((B, N), -1, dtype=torch.int64, device=dev),
           torch.full((B, N), np.nan, device=dev))
    per_level = tuple(torch.full_like(t, -7) for t in one)
    levels, n_off = [], 0
    for i, ((h, w), hd) in enumerate(zip(shapes, heads)):
        levels.append(dict(box=hd, ldbox=ld, cls=hd, ldcls=ld, anchors_wh=anchors[i], H=h, W=w, stride=strides[i], n_off=n_off))
        ops.decode(ops.DECODE_RAPID, hd, ld, per, 0, hd, ld, per, 6, 5, anchors[i], A, C, B, h, w, strides[i], (128, 96),
                   *per_level, n_off)
        n_off += A * h * w
    ops.decode_levels(ops.DECODE_RAPID, levels, per, 0, per, 6, 5, A, C, B, (128, 96), *one)
    for a, b in zip(one, per_level):
        assert torch.equal(a, b)


def _rot_inputs(b, rng):
    ang = (rng.random(b.shape[:-1], dtype=np.float32) * 360 - 180).astype(np.float32)
    return np.concatenate([b, ang[..., None]], -1)


def _check_rot_equals_plain(dev, b4, c, s, conf, nms, what):
    from mydetection_amd import ops
    rng = np.random.Generator(np.random.PCG64(b4.size))
    b5 = _rot_inputs(b4, rng)
    t4, t5 = torch.from_numpy(b4).to(dev), torch.from_numpy(b5).to(dev)
    tc, ts = torch.from_numpy(c).to(dev), torch.from_numpy(s).to(dev)
    plain, rot = ops.postprocess(t4, tc, ts, conf, nms), ops.postprocess(t5, tc, ts, conf, nms)
    assert rot['records'].shape[1] == ops._lib.REC_ROT_WORDS
    for k in ('count', 'bbox', 'score', 'class_idx', 'index'):
        assert torch.equal(plain[k], rot[k]), (what, k)
    dense4, dense5 = ops.postprocess_dense(t4, tc, ts, conf, nms), ops.postprocess_dense(t5, tc, ts, conf, nms)
    for k in ('count', 'score', 'class_idx', 'index'):
        assert torch.equal(dense4[k], dense5[k]) and torch.equal(dense4[k], plain[k]), (what, k)
    assert torch.equal(dense5['bbox'][..., :4], dense4['bbox']) and torch.equal(dense4['bbox'], plain['bbox'])
    counts = rot['count'].cpu().tolist()
    for i, k in enumerate(counts):
        idx = rot['index'][i, :k].long().cpu()
        want = torch.from_numpy(b5[i, :, 4])[idx]
        assert torch.equal(rot['angle'][i, :k].cpu(), want), what
        assert torch.equal(dense5['bbox'][i, :k, 4].cpu(), want), what
        assert not rot['angle'][i, k:].any() and not dense5['bbox'][i, k:].any()
    return counts


def test_rotated_postprocess_equals_the_plain_one(dev, golden):
    """Bit for bit on columns 0-3 with the angle gathered from the input: the reference's own post-process fixtures (top-k
    cut, ties at the cut, IoU at the threshold and one ulp either side, empty inputs) and a batch with > 512 passing
    candidates and a 200-way score tie."""
    g = golden('postprocess')
    for name in g['names']:
        b, c, s = g[f'{name}_in_bboxes'], g[f'{name}_in_cats'], g[f'{name}_in_scores']
        if not len(s):
            continue
        _check_rot_equals_plain(dev, b[None], c[None], s[None], float(g[f'{name}_conf']), float(g[f'{name}_nms']), str(name))
    rng = np.random.Generator(np.random.PCG64(3))
    B, N = 4, 12000
    b = np.empty((B, N, 4), np.float32)
    b[..., :2] = rng.random((B, N, 2), dtype=np.float32) * 1000
    b[..., 2:] = rng.random((B, N, 2), dtype=np.float32) * 90 + 2
    c = np.zeros((B, N), np.int64)
    c[1] = rng.integers(0, 5, size=N)
    s = rng.random((B, N), dtype=np.float32)
    s[2, 300:900] = s[2, 10]                               # a 600-way tie across the top-512 cut
    s[3] *= 0.001
    counts = _check_rot_equals_plain(dev, b, c, s, 0.3, 0.45, 'random')
    assert counts[0] > 100 and counts[3] == 0


def _model(dev, name):
    from mydetection_amd import synth
    from mydetection_amd.models.general import name_to_model
    m, cfg = name_to_model(name)
    m.load_state_dict(synth.make_state_dict(m.state_dict(), name), strict=True)
    return m.eval().to(dev), cfg


def _images(cfg, size, seed):
    from mydetection_amd import synth
    if cfg['general.input_format'] == 'RGB_1_norm':
        return synth.make_normalized_images(1, size, seed=seed)
    return synth.make_images(1, size, seed=seed)


def _check_detections(d, cand, g, what):
    """Detections at the fixture's three settings: equal to the reference's (count, classes, order; columns 0-3 and scores
    within 1e-4, angles within ANGLE_ATOL) where the fixture's decision margin exceeds twice the observed score error, and
    in every case equal to the oracle's post-process of THESE candidates on columns 0-3, with each angle its box's."""
    from oracle import postprocess as opp
    boxes, cats, scores, err = cand
    exact = 0
    for tag in ('ap', 'mid', 'demo'):
        conf, nms = float(g[f'pp_{tag}_conf']), float(g[f'pp_{tag}_nms'])
        r = d.post_process(conf, nms)
        assert r.bboxes.shape[1] == 5 and r._bb_format == 'cxcywhd'
        rb, rc, rs = r.bboxes.cpu().numpy(), r.cats.cpu().numpy(), r.scores.cpu().numpy()
        ob, oc, os_, src = opp.post_process(boxes[:, :4], cats, scores, conf, nms)
        np.testing.assert_array_equal(rc, oc, err_msg=f'{what} {tag}')
        np.testing.assert_array_equal(rs, os_, err_msg=f'{what} {tag}')
        np.testing.assert_array_equal(rb[:, :4], ob, err_msg=f'{what} {tag}')
        np.testing.assert_array_equal(rb[:, 4], boxes[src, 4], err_msg=f'{what} {tag}')
        if float(g[f'pp_{tag}_margin']) > 2 * err:
            exact += 1
            ref = g[f'pp_{tag}_bboxes_0']
            assert rb.shape == ref.shape, (what, tag, rb.shape, ref.shape)
            np.testing.assert_array_equal(rc, g[f'pp_{tag}_cats_0'])
            np.testing.assert_allclose(rs, g[f'pp_{tag}_scores_0'], rtol=RTOL, atol=ATOL)
            np.testing.assert_allclose(rb[:, :4], ref[:, :4], rtol=RTOL, atol=ATOL)
            np.testing.assert_allclose(rb[:, 4], ref[:, 4], rtol=0, atol=ANGLE_ATOL)
    return exact


@pytest.mark.parametrize('fixture', ['rapid_b1_256', 'd1_rapid_b1_256', 'rapid_b1_1024'])
def test_model_vs_reference_fixture(dev, golden, fixture):
    g = golden(fixture)
    name = str(g['config'])
    m, cfg = _model(dev, name)
    x = _images(cfg, int(g['size']), int(g['image_seed'])).to(dev)
    with torch.no_grad():
        d = m(x)[0]
    n = g['scores_0'].shape[0]
    assert d.bboxes.shape == (n, 5) and d._bb_format == 'cxcywhd'
    boxes, cats, scores = d.bboxes.cpu().numpy(), d.cats.cpu().numpy(), d.scores.cpu().numpy()
    np.testing.assert_allclose(scores, g['scores_0'], rtol=RTOL, atol=ATOL)
    ref = g['bboxes_0'] if 'bboxes_0' in g else g['bboxes_0_val']
    got = boxes if 'bboxes_0' in g else boxes[g['bboxes_0_idx']]
    np.testing.assert_allclose(got[:, :4], ref[:, :4], rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(got[:, 4], ref[:, 4], rtol=0, atol=ANGLE_ATOL)
    assert not cats.any() and not g['cats_0'].any()
    assert (scores >= 0.005).sum() >= 100 and (scores >= float(g['pp_demo_conf'])).sum() >= 5      # long-tailed scores
    assert boxes[:, 4].min() < -170 and boxes[:, 4].max() > 170                                    # angles over the full range
    err = float(np.abs(scores - g['scores_0']).max())
    _check_detections(d, (boxes, cats, scores, err), g, fixture)


@pytest.mark.parametrize('name', ['yv3_pl1_80', 'u5m_rapid', 'rapid_psl1'])
def test_other_rapid_configs_decode_their_own_heads(dev, name):
    """The three configurations without a model fixture: candidates equal the float64 restatement of RAPiDLayer on the
    head logits of this very forward, and the detections equal the oracle's post-process of these candidates."""
    m, cfg = _model(dev, name)
    x = _images(cfg, 256, 1).to(dev)
    with torch.no_grad():
        feats = m.fpn(m.backbone(x))
        raws = m.rpn(feats)
        d = m(x)[0]
    boxes, cats, scores = d.bboxes.cpu().numpy(), d.cats.cpu().numpy(), d.scores.cpu().numpy()
    parts = []
    for layer, raw in zip(m.det_layers, raws):
        cls = raw['class'].cpu().numpy() if layer.n_cls else np.zeros(raw['conf'].shape[:-1] + (0,), np.float32)
        parts.append(rapid_f64(raw['bbox'].cpu().numpy(), raw['conf'].cpu().numpy(), cls, layer.anchors.numpy(), layer.stride))
    rb, ri, rs = (np.concatenate([p[k] for p in parts], 1)[0] for k in range(3))
    np.testing.assert_allclose(boxes[:, :4], rb[:, :4], rtol=2e-6, atol=1e-4)
    np.testing.assert_allclose(boxes[:, 4], rb[:, 4], rtol=0, atol=1e-4)
    np.testing.assert_allclose(scores, rs, rtol=2e-6, atol=1e-9)
    if cfg['general.num_class']:
        assert len(np.unique(cats)) > 10
    from oracle import postprocess as opp
    r = d.post_process(cfg['test.ap_conf_thres'], cfg['test.nms_thres'])
    ob, oc, os_, src = opp.post_process(boxes[:, :4], cats, scores, cfg['test.ap_conf_thres'], cfg['test.nms_thres'])
    assert len(src) > 0
    np.testing.assert_array_equal(r.cats.cpu().numpy(), oc)
    np.testing.assert_array_equal(r.bboxes.cpu().numpy(), np.concatenate([ob, boxes[src, 4:5]], 1))


@pytest.mark.parametrize('name,lanes', [('rapid', 1), ('d1_rapid', 2)])
def test_graph_replay_equals_eager(dev, name, lanes):
    from mydetection_amd import synth
    from mydetection_amd.graph import GraphedPath
    m, cfg = _model(dev, name)
    x = torch.cat([_images(cfg, 256, s) for s in range(4)]).to(dev)
    gp = GraphedPath(m, x, 0.005, cfg['test.nms_thres'], lanes=lanes)
    assert gp.lanes == lanes
    rec = {k: v.clone() for k, v in gp(x).items()}
    eager = gp.eager(x)
    assert rec['records'].shape == (4, gp.records['records'].shape[1]) and 'angle' in rec
    for k in ('count', 'bbox', 'score', 'class_idx', 'index', 'angle'):
        assert torch.equal(rec[k], eager[k]), k
    assert int(rec['count'].min()) > 0
    x2 = x.flip(0).contiguous()
    rec2 = gp(x2)
    assert torch.equal(rec2['angle'], gp.eager(x2)['angle'])


def test_detector_predict_batch_and_json(dev, tmp_path):
    import PIL.Image
    from mydetection_amd import synth
    from mydetection_amd.api import Detector
    from mydetection_amd.models.general import name_to_model
    m, cfg = name_to_model('rapid')
    m.load_state_dict(synth.make_state_dict(m.state_dict(), 'rapid'), strict=True)
    det = Detector(model_and_cfg=(m.eval().cuda(), cfg))
    assert det.input_size == 1024 and det.conf_thres == 0.3 and det.nms_thres == 0.45
    imgs = []
    # one image per network input size, so that predict_batch's forward sees the same batch as detect_one's (a solo image
    # and the same image inside a batch differ in the last float bits) and the comparison can be bit for bit
    for i, (h, w) in enumerate([(300, 400), (250, 380), (400, 230)]):
        arr = (synth.make_images(1, max(h, w), seed=20 + i)[0, :, :h, :w].permute(1, 2, 0).numpy() * 255).astype(np.uint8)
        imgs.append(PIL.Image.fromarray(arr))
    kw = dict(input_size=512, conf_thres=0.05)
    batch = det.predict_batch(imgs, **kw)
    total = 0
    for img, got in zip(imgs, batch):
        one = det.detect_one(pil_img=img, **kw)
        assert got.bboxes.shape[1] == 5 and got.img_hw == (img.height, img.width)
        assert torch.equal(got.bboxes, one.bboxes) and torch.equal(got.scores, one.scores) and torch.equal(got.cats, one.cats)
        # original coordinates: columns 0-3 mapped back, the angle as the network produced it
        pre = [p for _, x, p, _ in det.preprocess_batch([img], **kw)]
        pad = pre[0][0]
        raw = det._records(next(det.preprocess_batch([img], **kw))[1], kw['conf_thres'], det.nms_thres)
        k = int(raw['count'][0])
        assert torch.equal(got.bboxes[:, 4], raw['angle'][0, :k])
        ori_w, ori_h, _, _, imw, imh = pad                   # utils/structures.py:175-189 with tl = (0, 0)
        want = raw['bbox'][0, :k].cpu().double().numpy() * np.array([ori_w / imw, ori_h / imh, ori_w / imw, ori_h / imh])
        np.testing.assert_allclose(got.bboxes[:, :4].cpu().numpy(), want, rtol=1e-5, atol=1e-4)
        js = got.to_json(5, eval_type='cxcywhd')
        assert [r['bbox'] for r in js] == got.bboxes.cpu().tolist() and all(r['category_id'] == 1 for r in js)
        total += len(got)
    assert total > 0
    from mydetection_amd.utils.structures import batched_to_json
    for idxs, rec in det._records_by_size(imgs, **kw):
        rows = batched_to_json(rec, [f'im{j}' for j in idxs], eval_type='cxcywhd')
        want = [r for j in idxs for r in batch[j].to_json(f'im{j}', eval_type='cxcywhd')]
        assert rows == want
        json.dumps(rows)
