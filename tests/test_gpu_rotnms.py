"""GPU tests of the rotated-IoU NMS (opt-in `rotated_nms`): the pairwise kernel and the post-process kernel's rotated
instance against the float64 checker tests/_rotbox_ref.py, which tests/test_rotnms_host.py ties to the reference through
tests/golden/rot_iou.npz.

IoU bar: 1e-5 absolute.  A float32 run of the clipping algorithm is within 1e-6 of float64 on boxes like the fixture's
and on coincident / parallel-edge pairs (observed on the MI355X: 4.8e-7 on the fixture), so the bar leaves room for another
sound formulation and none for a wrong one (the wrong angle convention alone is off by > 1e-2).  NMS decisions are compared exactly; every builder asserts that no
same-class pair of the selected candidates has a float64 IoU within 1e-4 (10 x the bar) of the threshold."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _rotbox_ref as chk  # noqa: E402
from test_rotnms_host import crafted_pairs, duplicate_pairs, thin_pairs  # noqa: E402

pytestmark = pytest.mark.gpu

IOU_ATOL = 1e-5
MARGIN = 1e-4


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda')


def _t(a, dev, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(dev)


def _run(dev, b, c, s, conf, nms, rotated):
    """(records dict, dense dict) as numpy, of the record and the dense entry point."""
    from mydetection_amd import ops
    args = (_t(b, dev), _t(c, dev, torch.int64), _t(s, dev))
    rec = ops.postprocess(*args, conf, nms, rotated_nms=rotated)
    dense = ops.postprocess_dense(*args, conf, nms, rotated_nms=rotated)
    torch.cuda.synchronize()
    return ({k: v.cpu().numpy() for k, v in rec.items() if k != 'records'}, {k: v.cpu().numpy() for k, v in dense.items()})


def _check_against_checker(dev, b, c, s, conf, nms, what):
    """The rotated post-process of a batch equals the checker image by image; returns the kept index lists."""
    rec, dense = _run(dev, b, c, s, conf, nms, True)
    kept = []
    for i in range(b.shape[0]):
        order = chk.select(c[i], s[i], conf)
        assert chk.margin(b[i], c[i], order, nms) >= MARGIN, f'{what}: image {i} has a pair at the threshold'
        want = chk.nms(b[i], c[i], s[i], conf, nms)
        k = int(rec['count'][i])
        assert k == len(want), (what, i, k, len(want))
        np.testing.assert_array_equal(rec['index'][i, :k], want, err_msg=f'{what} image {i}')
        # boxes, angles, classes and scores are copies of the inputs, bit for bit; slots past the count are zero
        np.testing.assert_array_equal(rec['bbox'][i, :k].view(np.uint32), b[i][want, :4].view(np.uint32))
        np.testing.assert_array_equal(rec['angle'][i, :k].view(np.uint32), b[i][want, 4].view(np.uint32))
        np.testing.assert_array_equal(rec['score'][i, :k].view(np.uint32), s[i][want].view(np.uint32))
        np.testing.assert_array_equal(rec['class_idx'][i, :k], c[i][want])
        for f in ('bbox', 'angle', 'score', 'class_idx', 'index'):
            assert not rec[f][i, k:].any(), (what, i, f)
        # the dense entry point agrees with the record entry point
        assert int(dense['count'][i]) == k
        np.testing.assert_array_equal(dense['bbox'][i].view(np.uint32),
                                      np.concatenate([rec['bbox'][i], rec['angle'][i][:, None]], 1).view(np.uint32))
        for f in ('score', 'class_idx', 'index'):
            np.testing.assert_array_equal(dense[f][i], rec[f][i])
        kept.append(want.tolist())
    return kept


def test_pairwise_kernel_on_the_reference_fixture(dev, golden):
    from mydetection_amd.utils.bbox_ops import iou_rotated
    g = golden('rot_iou')
    b = _t(g['boxes'], dev)
    got = iou_rotated(b, b)
    assert got.dtype == torch.float32 and got.shape == (24, 24) and got.is_cuda
    got = got.cpu().numpy().astype(np.float64)
    err = np.abs(got - g['exact_iou']).max()
    off = ~np.eye(24, dtype=bool)
    mask_err = np.abs(got - g['mask_iou'])[off].max()
    print(f'pairwise kernel vs float64 exact: max {err:.3e}; vs the reference mask IoU: max {mask_err:.3e}')
    assert err <= IOU_ATOL
    assert mask_err <= float(g['mask_vs_exact_max']) + IOU_ATOL


def test_crafted_pairs(dev):
    from mydetection_amd.utils.bbox_ops import iou_rle, iou_rotated, nms_rotbb
    pairs = crafted_pairs() + thin_pairs()
    a = np.array([p[1] for p in pairs], np.float32)
    b = np.array([p[2] for p in pairs], np.float32)
    want = np.array([p[3] for p in pairs])
    got = iou_rotated(_t(a, dev), _t(b, dev)).cpu().numpy()
    for i, p in enumerate(pairs):
        assert abs(float(got[i, i]) - want[i]) <= IOU_ATOL, (p[0], got[i, i])
        if want[i] == 0:
            assert got[i, i] == 0, p[0]
    # every pair of the whole set, both ways round, against the checker
    np.testing.assert_allclose(got, chk.iou_matrix(a, b), rtol=0, atol=IOU_ATOL)
    np.testing.assert_allclose(iou_rotated(_t(b, dev), _t(a, dev)).cpu().numpy(), chk.iou_matrix(b, a), rtol=0, atol=IOU_ATOL)
    # cancellation: small boxes far from the origin
    far = np.array([[2000, 2000, 10, 6, 20], [2003, 2000, 10, 6, 20]], np.float32)
    g = iou_rotated(_t(far[:1], dev), _t(far[1:], dev)).cpu().numpy()[0, 0]
    ref = chk.iou_pairs(far[:1], far[1:])[0]
    assert 0.3 < ref < 0.6 and abs(float(g) - ref) <= IOU_ATOL, (g, ref)
    # degenerate boxes: zero area against a real box is exactly 0; 0/0 is NaN and never suppresses
    zero = np.array([[50, 50, 0, 10, 0]], np.float32)
    real = np.array([[50, 50, 20, 10, 0]], np.float32)
    assert iou_rotated(_t(zero, dev), _t(real, dev)).cpu().numpy()[0, 0] == 0
    assert iou_rotated(_t(real, dev), _t(zero, dev)).cpu().numpy()[0, 0] == 0
    assert np.isnan(iou_rotated(_t(zero, dev), _t(zero, dev)).cpu().numpy()[0, 0])
    # ... also when the box without area is rotated and only partly inside (its doubled edge crosses the real box)
    rng = np.random.Generator(np.random.PCG64(2))
    n = 512
    real = np.concatenate([rng.uniform(100, 200, (n, 2)), rng.uniform(20, 100, (n, 2)), rng.uniform(-180, 180, (n, 1))], 1).astype(np.float32)
    flat = np.concatenate([real[:, :2] + rng.normal(0, 20, (n, 2)), np.zeros((n, 1)), rng.uniform(20, 100, (n, 1)),
                           rng.uniform(-180, 180, (n, 1))], 1).astype(np.float32)
    flat[::2, 2:4] = flat[::2, 3:1:-1]                                          # h = 0 on every other one
    assert not iou_rotated(_t(real, dev), _t(flat, dev)).cpu().numpy().any()
    assert not iou_rotated(_t(flat, dev), _t(real, dev)).cpu().numpy().any()
    both = torch.from_numpy(np.concatenate([zero, zero]))
    assert nms_rotbb(both, torch.tensor([0.9, 0.8]), nms_thres=0.3).tolist() == [0, 1]
    # the reference-named wrapper: 1-d inputs, numpy inputs, an empty set, the input's device
    one = iou_rle(torch.from_numpy(a[6]), torch.from_numpy(b[6]), img_size=1024)
    assert one.shape == (1, 1) and one.dtype == torch.float32 and not one.is_cuda and abs(float(one) - 400 / 7600) <= IOU_ATOL
    arr = iou_rle(a[6], b[6:8], img_hw=(512, 512), return_numpy=True)
    assert isinstance(arr, np.ndarray) and arr.shape == (1, 2) and arr.dtype == np.float32
    assert iou_rle(_t(a[:1], dev), torch.zeros(0, 5, device=dev)).shape == (1, 0)
    assert iou_rle(_t(a[:3], dev), _t(b[:2], dev)).is_cuda


@pytest.mark.parametrize('thin', [False, True], ids=['5-350px', 'thin'])
def test_duplicates_sweep(dev, thin):
    """2 048 seeded pairs of one rectangle written twice (exactly, or with sub-pixel jitter; turned by multiples of 90 degrees
    with w and h swapped) at the IoU bar, plus the pairs for which a vertex list capped at one more vertex per stage returned
    1/3.  Coincident edges put corners on the clip boundary within round-off; every vertex has to survive that.
    The thin set goes to 49 : 1 (6 x 295 px).  The float32 half-extent vectors carry a direction error of ~1e-7 rad, which
    moves the IoU of a duplicate by about that times L / W -- 5e-6 at 49 : 1 -- so the 1e-5 bar holds up to there and the
    shapes stop there."""
    from mydetection_amd.utils.bbox_ops import iou_rotated, nms_rotbb
    a, b, exact = duplicate_pairs(3, 2048, thin)
    extra = np.array([[[1082.2076, 554.8906, 29.681957, 44.07503, -150.89903], [1082.2076, 554.8906, 44.07503, 29.681957, 119.10097]],
                      [[694.12695, 221.60498, 322.60315, 53.38791, 110.31072], [694.12695, 221.60498, 53.38791, 322.60315, 380.31073]],
                      [[234.88892, 810.4534, 338.66672, 265.32062, -55.435104], [234.88892, 810.4534, 338.66672, 265.32062, -55.435104]]],
                     np.float32)
    a, b = np.concatenate([extra[:, 0], a]), np.concatenate([extra[:, 1], b])
    want = chk.iou_pairs(a, b)
    got = torch.diagonal(iou_rotated(_t(a, dev), _t(b, dev))).cpu().numpy().astype(np.float64)
    back = torch.diagonal(iou_rotated(_t(b, dev), _t(a, dev))).cpu().numpy().astype(np.float64)
    err = max(np.abs(got - want).max(), np.abs(back - want).max())
    print(f'duplicates ({"thin" if thin else "5-350 px"}): max |kernel - float64| {err:.3e}, smallest IoU of an exact duplicate '
          f'{min(got[3:][exact].min(), back[3:][exact].min()):.7f}')
    assert err <= IOU_ATOL
    # through the NMS: 256 rectangles 800 px apart, each followed by its duplicate with a lower score -- one of each stays
    n = 256
    a2, b2 = a[3:3 + n].copy(), b[3:3 + n].copy()
    grid = np.stack([np.arange(n) % 16, np.arange(n) // 16], 1).astype(np.float32) * 800 + 400
    b2[:, :2] += grid - a2[:, :2]
    a2[:, :2] = grid
    boxes = np.concatenate([a2, b2])
    scores = np.concatenate([np.linspace(0.9, 0.6, n), np.linspace(0.5, 0.2, n)]).astype(np.float32)
    keep = nms_rotbb(_t(boxes, dev), _t(scores, dev), nms_thres=0.45)
    assert keep.tolist() == list(range(n))


def _decision_batch(seed):
    """B = 2, N = 600, 3 classes: clusters of rotated near-duplicates; image 0 has 560 candidates above conf (the top-512
    cut runs), image 1 has 40.  Candidates 0-3 of both images are the two pairs rotation decides (class 2, top scores):
    0/1 cross at 45 / 135 degrees on one centre, 2/3 are one rectangle written two ways, with EQUAL scores."""
    rng = np.random.Generator(np.random.PCG64(seed))
    B, N, conf = 2, 600, 0.3
    b = np.empty((B, N, 5), np.float32)
    c = np.empty((B, N), np.int64)
    s = np.empty((B, N), np.float32)
    for i, npass in enumerate((560, 40)):
        K = 45 if i == 0 else 12
        ctr = rng.uniform(100, 1500, size=(K, 2))
        wh = rng.uniform(30, 160, size=(K, 2))
        ang = rng.uniform(-180, 180, size=K)
        kc = rng.integers(0, 2, size=K)
        k = rng.integers(0, K, size=N)
        b[i, :, :2] = ctr[k] + rng.normal(0, 6, size=(N, 2))
        b[i, :, 2:4] = wh[k] * (1 + rng.normal(0, 0.08, size=(N, 2)))
        b[i, :, 4] = ang[k] + rng.normal(0, 8, size=N) + 90 * rng.integers(0, 4, size=N) * (rng.random(N) < 0.2)
        c[i] = kc[k]
        s[i] = rng.uniform(0.0, conf * 0.99, size=N)
        passing = rng.permutation(np.arange(4, N))[:npass - 4]
        s[i, passing] = rng.uniform(conf, 0.9, size=npass - 4)
        b[i, 0] = (3000, 3000, 200, 20, 45)
        b[i, 1] = (3000, 3000, 200, 20, 135)
        b[i, 2] = (3500, 3000, 200, 20, 0)
        b[i, 3] = (3500, 3000, 20, 200, 90)
        c[i, :4] = 2
        s[i, :4] = (0.99, 0.98, 0.97, 0.97)
    return b, c, s, conf


def test_nms_decisions(dev):
    b, c, s, conf = _decision_batch(8)
    nms = 0.45
    assert (s[0] >= conf).sum() == 560 and (s[1] >= conf).sum() == 40
    kept = _check_against_checker(dev, b, c, s, conf, nms, 'decisions')
    rec_al, _ = _run(dev, b, c, s, conf, nms, False)
    for i in range(2):
        assert (30, 5)[i] < len(kept[i]) < (500, 40)[i]                      # clusters were merged, not everything
        al = rec_al['index'][i, :int(rec_al['count'][i])].tolist()
        # crossed thin boxes: both stay under the rotated IoU (0.05); the axis-aligned kernel sees one box twice
        assert 0 in kept[i] and 1 in kept[i] and 0 in al and 1 not in al
        # one rectangle written two ways: the rotated IoU is 1, the tie goes to the lower index; axis-aligned IoU 0.05
        assert 2 in kept[i] and 3 not in kept[i] and 2 in al and 3 in al


def test_ge_rule_at_the_threshold(dev):
    b = np.array([[[50, 50, 20, 10, 0], [50, 50, 20, 10, 0]]], np.float32)       # IoU exactly 1.0 in float32
    c = np.zeros((1, 2), np.int64)
    s = np.array([[0.9, 0.8]], np.float32)
    rot, _ = _run(dev, b, c, s, 0.1, 1.0, True)
    al, _ = _run(dev, b, c, s, 0.1, 1.0, False)
    assert int(rot['count'][0]) == 1 and rot['index'][0, 0] == 0                 # IoU >= 1.0: suppressed
    assert int(al['count'][0]) == 2                                              # IoU > 1.0: kept


def test_angle_zero_reduces_to_the_axis_aligned_kernel(dev):
    rng = np.random.Generator(np.random.PCG64(12))
    N, nms = 300, 0.45
    b = np.zeros((1, N, 5), np.float32)
    b[0, :, :2] = rng.uniform(0, 250, size=(N, 2))
    b[0, :, 2:4] = rng.uniform(20, 110, size=(N, 2))
    c = rng.integers(0, 2, size=(1, N))
    s = rng.random((1, N), dtype=np.float32)
    order = chk.select(c[0], s[0], 0.0)
    assert chk.margin(b[0], c[0], order, nms) >= MARGIN
    assert chk.margin(b[0], c[0], order, nms, iou=chk.aligned_iou_matrix) >= MARGIN
    rot, _ = _run(dev, b, c, s, 0.0, nms, True)
    al, _ = _run(dev, b, c, s, 0.0, nms, False)
    k = int(rot['count'][0])
    assert k == int(al['count'][0]) and 50 < k < 250
    np.testing.assert_array_equal(rot['index'], al['index'])
    np.testing.assert_array_equal(rot['index'][0, :k], chk.nms(b[0], c[0], s[0], 0.0, nms))


def test_chain_takes_the_sequential_fallback(dev):
    """30 boxes in a row, each overlapping only its neighbours above the threshold (IoU 0.6; next but one 0.33), scores
    falling along the chain: box 2t is kept because 2t-1 went because 2t-2 was kept ... -- a dependency chain of 30, more
    than the 12 fixed-point rounds, so the selection runs in its sequential form."""
    n, ang = 30, 30.0
    step = 10.0 * np.array([np.cos(np.deg2rad(ang)), np.sin(np.deg2rad(ang))])
    b = np.zeros((1, n, 5), np.float32)
    b[0, :, :2] = np.array([300.0, 200.0]) + np.arange(n)[:, None] * step
    b[0, :, 2:] = (40, 20, ang)
    c = np.zeros((1, n), np.int64)
    s = np.linspace(0.9, 0.3, n, dtype=np.float32)[None]
    m = chk.iou_matrix(b[0], b[0])
    assert abs(m[0, 1] - 0.6) < 1e-3 and abs(m[0, 2] - 1 / 3) < 1e-3
    kept = _check_against_checker(dev, b, c, s, 0.1, 0.45, 'chain')
    assert kept[0] == list(range(0, n, 2))


def test_footprint_and_empty_input(dev):
    from mydetection_amd import _lib, ops
    from mydetection_amd.utils.bbox_ops import nms_rotbb
    b, c, s, conf = _decision_batch(8)
    B, words, guard = 2, _lib.REC_ROT_WORDS, 64
    buf = torch.full((2 * guard + B * words,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    rec = ops.postprocess(_t(b, dev), _t(c, dev, torch.int64), _t(s, dev), conf, 0.45,
                          records=buf[guard:guard + B * words].view(B, words), rotated_nms=True)
    torch.cuda.synchronize()
    assert (buf[:guard] == 0x5A5A5A5A).all() and (buf[-guard:] == 0x5A5A5A5A).all()
    assert int(rec['count'][0]) > 0 and rec['records'].data_ptr() == buf[guard:].data_ptr()
    # the pairwise output: Na x Nb floats and nothing else (sizes that are no multiple of the block)
    na, nb = 37, 29
    a5, b5 = _t(b[0, :na], dev), _t(b[0, 100:100 + nb], dev)
    out = torch.full((2 * guard + na * nb,), float('nan'), dtype=torch.float32, device=dev)
    code = _lib.lib().mydet_rotated_iou_f32(ops._ptr(a5), na, ops._ptr(b5), nb, ops._ptr(out[guard:]), ops._stream())
    assert code == 0
    torch.cuda.synchronize()
    assert torch.isnan(out[:guard]).all() and torch.isnan(out[-guard:]).all()
    got = out[guard:guard + na * nb].view(na, nb).cpu().numpy()
    np.testing.assert_allclose(got, chk.iou_matrix(b[0, :na], b[0, 100:100 + nb]), rtol=0, atol=IOU_ATOL)
    keep = nms_rotbb(torch.zeros(0, 5, device=dev), torch.zeros(0, device=dev))
    assert keep.dtype == torch.int64 and keep.shape == (0,) and keep.is_cuda
    # nms_rotbb returns indices in score order
    keep = nms_rotbb(_t(b[1, :60], dev), _t(s[1, :60], dev), nms_thres=0.45)
    want = chk.nms(b[1, :60], np.zeros(60, np.int64), s[1, :60], -np.inf, 0.45)
    assert keep.dtype == torch.int64 and keep.tolist() == want.tolist()


def test_model_level_rotated_nms(dev, golden):
    import PIL.Image
    from mydetection_amd import synth
    from mydetection_amd.api import Detector
    from mydetection_amd.models.general import name_to_model
    g = golden('rapid_b1_256')
    m, cfg = name_to_model('rapid')
    m.load_state_dict(synth.make_state_dict(m.state_dict(), 'rapid'), strict=True)
    m = m.eval().to(dev)
    size = int(g['size'])
    x = synth.make_images(1, size, seed=int(g['image_seed'])).to(dev)
    with torch.no_grad():
        d = m(x)[0]
    boxes, cats, scores = d.bboxes.cpu().numpy(), d.cats.cpu().numpy(), d.scores.cpu().numpy()
    conf = 0.005
    order = chk.select(cats, scores, conf)
    assert len(order) >= 100
    margins = {t: chk.margin(boxes, cats, order, t) for t in (0.45, 0.4, 0.5)}
    usable = [t for t, v in margins.items() if v >= MARGIN]
    assert usable, f'every threshold has a pair within {MARGIN} of it: {margins}'
    nms = usable[0]
    want = chk.nms(boxes, cats, scores, conf, nms)
    r = d.post_process(conf, nms, rotated_nms=True)
    assert r._bb_format == 'cxcywhd' and len(r) == len(want) > 0
    np.testing.assert_array_equal(r.bboxes.cpu().numpy().view(np.uint32), boxes[want].view(np.uint32))
    np.testing.assert_array_equal(r.scores.cpu().numpy().view(np.uint32), scores[want].view(np.uint32))
    r2 = r.nms(nms, rotated=True)                           # the survivors again: no pair is left to suppress
    assert torch.equal(r2.bboxes, r.bboxes) and torch.equal(r2.scores, r.scores)
    # Detector: eager, then a captured graph, then the default flag again
    det = Detector(model_and_cfg=(m, cfg))
    arr = (synth.make_images(1, size, seed=int(g['image_seed']))[0].permute(1, 2, 0).numpy() * 255).astype(np.uint8)
    imgs = [PIL.Image.fromarray(arr)]

    def fields(o):
        return o.bboxes.clone(), o.scores.clone(), o.cats.clone()
    # what the rotated NMS must keep on the Detector's own input: the checker on the candidates of that input
    xin = next(det.preprocess_batch(imgs, input_size=size))[1]
    with torch.no_grad():
        cb, cc, cs = (t[0].cpu().numpy() for t in m.forward_candidates(xin))
    dorder = chk.select(cc, cs, conf)
    dmargins = {t: chk.margin(cb, cc, dorder, t) for t in (0.45, 0.4, 0.5)}
    usable = [t for t, v in dmargins.items() if v >= MARGIN]
    assert usable, f'every threshold has a pair within {MARGIN} of it on the Detector input: {dmargins}'
    nms = usable[0]
    kw = dict(input_size=size, conf_thres=conf, nms_thres=nms)
    dwant = chk.nms(cb, cc, cs, conf, nms)
    dplain = chk.nms(cb, cc, cs, conf, nms, iou=chk.aligned_iou_matrix, strict=True)
    assert dwant.tolist() != dplain.tolist(), 'rotation decides nothing on this input: the test would show nothing'
    base = fields(det.predict_batch(imgs, **kw)[0])
    eager = fields(det.predict_batch(imgs, rotated_nms=True, **kw)[0])
    np.testing.assert_array_equal(eager[1].cpu().numpy().view(np.uint32), cs[dwant].view(np.uint32))
    np.testing.assert_array_equal(eager[0][:, 4].cpu().numpy().view(np.uint32), cb[dwant, 4].view(np.uint32))
    assert not (len(base[1]) == len(eager[1]) and torch.equal(base[1], eager[1])), 'the flag changed nothing'
    assert not any(k[3] for k in det._graphs.graphs)
    replay = fields(det.predict_batch(imgs, rotated_nms=True, **kw)[0])
    assert [k[3] for k in det._graphs.graphs] == [True], 'the second rotated call replays a captured graph'
    for a, b in zip(eager, replay):
        assert torch.equal(a, b)
    one = det.detect_one(pil_img=imgs[0], rotated_nms=True, **kw)
    assert torch.equal(one.bboxes, eager[0])
    for _ in range(2):                                       # eager again, then a graph of its own
        again = fields(det.predict_batch(imgs, **kw)[0])
        for a, b in zip(base, again):
            assert torch.equal(a, b)
    assert sorted(k[3] for k in det._graphs.graphs) == [False, True]
    assert len(eager[0]) > 0 and eager[0].shape[1] == 5
