"""GPU: the NMS modes of postprocess_kernel (include/mydet.h, "NMS modes": class-agnostic suppression, Soft-NMS, box merging)
against the numpy restatement in tests/_nms_ref.py, and `nms=` through ops, ImageObjects and the Detector.

Every comparison with the reference is `==`: the count, the classes, the candidate indices, the bits of the scores and the bits
of the boxes.  That is legitimate for the Gaussian kind because of the seed condition tests/test_nms_modes_host.py asserts for
the inputs used here (tests/_nms_cases.py): every weight is far enough from a float32 rounding midpoint that two correct
double-precision exp agree after rounding.  The linear decay and the merge use only +, -, *, / in float32 and float64.

  launch (tests/_nms_cases.py)   what it is for
  -----------------------------  ---------------------------------------------------------------------------------------------
  N1, N63, N64, N65              one box; a group that ends one short of, on and one past a wave's 64 lanes
  N600                           more than 512 pass: the top-k boundary feeds the mode; 80 classes; class id 4095
  N512                           one class of 512 boxes, min_score 0: 512 dependent picks in one wave (8 boxes a lane); an empty
                                 image; 256 of 512 passing
  N65_min_score                  every group's first pick is below min_score: the soft kinds emit nothing
Each with and without `agnostic`, for boxes of width 4 and 5 (merge on width 5 is MYDET_E_UNSUPP)."""
import ctypes

import numpy as np
import pytest
import torch

import _nms_cases as nc
import _nms_ref as ref
from _arena import SENTINEL_BITS, flat_arena
from mydetection_amd import ops
from mydetection_amd.api import Nms

pytestmark = pytest.mark.gpu

FIELDS = ('bbox', 'score', 'class_idx', 'index')
CASES = [(n, k, a, w) for n in nc.NAMES for k, a in nc.MODES for w in (4, 5) if not (k == 'merge' and w == 5)]


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    from mydetection_amd import _lib
    _lib.lib()                                   # fail loudly if the HIP library is missing
    return torch.device('cuda:0')


def _inputs(L, dev, width=4):
    b = np.stack([img['b'] for img in L['images']])
    if width == 5:
        b = np.concatenate([b, np.stack([img['angle'] for img in L['images']])[..., None]], axis=2)
    c = np.stack([img['c'] for img in L['images']])
    s = np.stack([img['s'] for img in L['images']])
    return torch.from_numpy(b).to(dev), torch.from_numpy(c).to(dev), torch.from_numpy(s).to(dev)


def _nms(L, kind, agn):
    return Nms(kind, agn, nc.SIGMA, L['min_score'])


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _host(out, i):
    """Image i of a record dict (or of the dense outputs) as host arrays; a rotated record's angle becomes box column 4."""
    bbox = out['bbox'][i].cpu().numpy()
    if 'angle' in out:
        bbox = np.concatenate([bbox, out['angle'][i].cpu().numpy()[:, None]], axis=1)
    return dict(count=int(out['count'][i]), bbox=bbox, score=out['score'][i].cpu().numpy(), class_idx=out['class_idx'][i].cpu().numpy(),
                index=out['index'][i].cpu().numpy())


def _check_image(img, want, got, what):
    k = want['count']
    assert got['count'] == k, f"{what}: {got['count']} detections, the reference has {k}"
    np.testing.assert_array_equal(got['index'][:k].astype(np.int64), want['index'], err_msg=f'{what}: candidate indices / order')
    np.testing.assert_array_equal(got['class_idx'][:k], want['cls'], err_msg=what)
    np.testing.assert_array_equal(_bits(got['score'][:k]), _bits(want['score']), err_msg=f'{what}: score bits')
    np.testing.assert_array_equal(_bits(got['bbox'][:k, :4]), _bits(want['bbox'][:, :4]), err_msg=f'{what}: box bits')
    if got['bbox'].shape[1] == 5:
        np.testing.assert_array_equal(_bits(got['bbox'][:k, 4]), _bits(img['angle'][want['index']]), err_msg=f'{what}: the angle travels')
    for f in FIELDS:
        assert not _bits(got[f][k:]).any(), f'{what}: {f} rows past the count are not zero'


def test_the_cases_take_every_branch():
    nc.check_branches()


@pytest.mark.parametrize('name,kind,agn,width', CASES)
def test_modes_against_the_reference(dev, name, kind, agn, width):
    L = nc.launches()[name]
    want, _ = nc.expected(name, kind, agn)
    tb, tc, ts = _inputs(L, dev, width)
    assert tb.shape[0] <= 4
    rec = ops.postprocess(tb, tc, ts, L['conf'], L['thr'], nms=_nms(L, kind, agn))
    dense = ops.postprocess_dense(tb, tc, ts, L['conf'], L['thr'], nms=_nms(L, kind, agn))
    assert ('angle' in rec) == (width == 5) and dense['bbox'].shape[2] == width
    for i, img in enumerate(L['images']):
        what = f"{name}/{img['name']} {kind} agnostic={agn} width {width}"
        _check_image(img, want[i], _host(rec, i), what + ' (records)')
        _check_image(img, want[i], _host(dense, i), what + ' (dense)')


@pytest.mark.parametrize('topk', [1, 64, 200])
def test_runtime_topk_feeds_the_mode(dev, topk):
    """The dense entry point with topk < 512: the selected list is the topk best, rows topk.. do not exist."""
    L = nc.launches()['N600']
    tb, tc, ts = _inputs(L, dev)
    for kind, agn in (('soft-linear', True), ('merge', False), ('hard', True)):
        dense = ops.postprocess_dense(tb, tc, ts, L['conf'], L['thr'], topk=topk, nms=_nms(L, kind, agn))
        for i, img in enumerate(L['images']):
            want = ref.run(img['b'], img['c'], img['s'], L['conf'], L['thr'], kind, agn, nc.SIGMA, L['min_score'], topk=topk)
            got = _host(dense, i)
            assert len(got['score']) == topk
            _check_image(img, want, got, f'topk {topk} {kind} {agn}')


def test_bad_class_id_fails_the_image(dev):
    """A selected class id outside [0, 4096) gives count -1 and zero rows in every mode, the neighbour image is untouched."""
    L = nc.launches()['N65']
    tb, tc, ts = _inputs(L, dev)
    tc = tc.clone()
    tc[0, int(ts[0].argmax())] = 4096
    for kind, agn in nc.MODES:
        rec = ops.postprocess(tb, tc, ts, L['conf'], L['thr'], nms=_nms(L, kind, agn))
        got = _host(rec, 0)
        assert got['count'] == -1 and not any(_bits(got[f]).any() for f in FIELDS), (kind, agn)
        _check_image(L['images'][1], nc.expected('N65', kind, agn)[0][1], _host(rec, 1), f'neighbour {kind} {agn}')


@pytest.mark.parametrize('width', [4, 5])
def test_plain_hard_through_the_new_entry_points_is_the_shipped_call(dev, width):
    for name in ('N65', 'N600', 'N512'):
        L = nc.launches()[name]
        tb, tc, ts = _inputs(L, dev, width)
        old = ops.postprocess(tb, tc, ts, L['conf'], L['thr'])
        new = ops.postprocess(tb, tc, ts, L['conf'], L['thr'], nms=Nms('hard', agnostic=False))
        assert torch.equal(old['records'], new['records']), f'{name}: records differ'
        old = ops.postprocess_dense(tb, tc, ts, L['conf'], L['thr'], topk=300)
        new = ops.postprocess_dense(tb, tc, ts, L['conf'], L['thr'], topk=300, nms=Nms())
        for f in ('count',) + FIELDS:
            assert torch.equal(old[f].view(torch.int32 if old[f].dtype == torch.float32 else old[f].dtype),
                               new[f].view(torch.int32 if new[f].dtype == torch.float32 else new[f].dtype)), f'{name}: dense {f} differs'
        assert int(old['count'].sum()) > 0


def _mode(kind, agnostic=0, sigma=0.5, min_score=0.25):
    from mydetection_amd import _lib
    return _lib.NmsMode(kind, agnostic, sigma, min_score, 0)


def test_rejected_modes_launch_nothing(dev):
    """Every MYDET_E_BADARG and MYDET_E_UNSUPP of the mode rules, through the four entry points: the code comes back and the
    outputs keep their canary."""
    from mydetection_amd import _lib
    from mydetection_amd.ops import _ptr, _stream
    lib = _lib.lib()
    B, N = 1, 16
    ts = torch.ones((B, N), device=dev)
    tc = torch.zeros((B, N), dtype=torch.int64, device=dev)
    scratch = torch.empty((B, N), dtype=torch.int64, device=dev)
    nan, inf = float('nan'), float('inf')
    H, L_, G, M = _lib.NMS_HARD, _lib.NMS_SOFT_LINEAR, _lib.NMS_SOFT_GAUSSIAN, _lib.NMS_MERGE
    # (mode or None, conf_thres, code for width 4, code for width 5)
    rejected = [(None, 0.5, -1, -1), (_mode(-1), 0.5, -1, -1), (_mode(4), 0.5, -1, -1), (_mode(H, 2), 0.5, -1, -1), (_mode(H, -1), 0.5, -1, -1),
                (_mode(L_), -0.5, -1, -1), (_mode(L_), nan, -1, -1), (_mode(L_), -inf, -1, -1), (_mode(G), -0.5, -1, -1),
                (_mode(L_, min_score=-0.1), 0.5, -1, -1), (_mode(G, min_score=nan), 0.5, -1, -1),
                (_mode(G, sigma=0.0), 0.5, -1, -1), (_mode(G, sigma=-1.0), 0.5, -1, -1), (_mode(G, sigma=nan), 0.5, -1, -1),
                (_mode(M), 0.0, -1, -1), (_mode(M), -0.5, -1, -1), (_mode(M), nan, -1, -1), (_mode(M, 1), 0.0, -1, -1),
                (_mode(M), 0.5, 0, -2), (_mode(M, 1), 0.5, 0, -2)]
    for width in (4, 5):
        tb = torch.ones((B, N, width), device=dev)
        words = _lib.REC_WORDS if width == 4 else _lib.REC_ROT_WORDS
        dense_fn = lib.mydet_postprocess_nms_f32 if width == 4 else lib.mydet_postprocess_rot_nms_f32
        rec_fn = lib.mydet_postprocess_records_nms_f32 if width == 4 else lib.mydet_postprocess_records_rot_nms_f32
        for mode, conf, code4, code5 in rejected:
            code = code4 if width == 4 else code5
            if code == 0:
                continue
            outs = [torch.full((B * 512 * w,), SENTINEL_BITS, dtype=torch.int32, device=dev) for w in (1, width, 2, 1, 1)]
            records = torch.full((B, words), SENTINEL_BITS, dtype=torch.int32, device=dev)
            mp = None if mode is None else ctypes.byref(mode)
            what = (width, None if mode is None else (mode.kind, mode.agnostic, mode.sigma, mode.min_score), conf)
            assert dense_fn(_ptr(tb), _ptr(tc), _ptr(ts), B, N, conf, 0.45, 512, mp, *(_ptr(o) for o in outs), _ptr(scratch), _stream()) == code, what
            assert rec_fn(_ptr(tb), _ptr(tc), _ptr(ts), B, N, conf, 0.45, mp, _ptr(records), _ptr(scratch), _stream()) == code, what
            torch.cuda.synchronize()
            assert all(bool((o == SENTINEL_BITS).all()) for o in outs + [records]), what
    # the same buffers are a valid call: 16 copies of one box
    tb = torch.ones((B, N, 4), device=dev)
    records = torch.full((B, _lib.REC_WORDS), SENTINEL_BITS, dtype=torch.int32, device=dev)
    for mode, count in ((_mode(H, 1), 1), (_mode(M), 1), (_mode(L_, min_score=0.0), 16), (_mode(G, min_score=0.5), 1)):
        assert lib.mydet_postprocess_records_nms_f32(_ptr(tb), _ptr(tc), _ptr(ts), B, N, 0.5, 0.45, ctypes.byref(mode), _ptr(records),
                                                     _ptr(scratch), _stream()) == 0
        torch.cuda.synchronize()
        assert int(records[0, 0]) == count, (mode.kind, int(records[0, 0]))
    # the tile merge: agnostic outside {0, 1} is BADARG, agnostic with rotated_nms UNSUPP; nothing is written
    T = 2
    tiles = torch.zeros((T * B, _lib.REC_ROT_WORDS), dtype=torch.int32, device=dev)
    org = torch.zeros((T, 2), dtype=torch.int32, device=dev)
    nbytes = lib.mydet_merge_tile_records_scratch_bytes(B, T, 5)
    mscratch = torch.empty(nbytes // 8, dtype=torch.int64, device=dev)
    out = torch.full((B, _lib.REC_ROT_WORDS), SENTINEL_BITS, dtype=torch.int32, device=dev)
    for agnostic, rotated, code in ((2, 0, -1), (-1, 0, -1), (1, 1, -2)):
        assert lib.mydet_merge_tile_records_nms_f32(_ptr(tiles), B * _lib.REC_ROT_WORDS, _lib.REC_ROT_WORDS, B, T, 5, _ptr(org), 0.45,
                                                    _lib.MERGE_IOU, rotated, agnostic, _ptr(out), _ptr(mscratch), nbytes, _stream()) == code
    torch.cuda.synchronize()
    assert bool((out == SENTINEL_BITS).all())


@pytest.mark.parametrize('kind,agn,width', [(k, a, w) for k, a in nc.MODES for w in (4, 5) if not (k == 'merge' and w == 5)])
def test_footprint(dev, kind, agn, width):
    """records and scratch between sentinel guard bands: the bands are untouched and every word of the B records is written."""
    from mydetection_amd import _lib
    L = nc.launches()['N600']
    tb, tc, ts = _inputs(L, dev, width)
    B, N = ts.shape
    words = ops.record_words(width)
    out, chk_out = flat_arena(B * words, dev)
    scratch, chk_scratch = flat_arena(B * N * 2, dev)                            # B * N * 8 bytes
    mode = ops.nms_mode('test', _nms(L, kind, agn), L['conf'], width)
    fn = getattr(_lib.lib(), 'mydet_postprocess_records_nms_f32' if width == 4 else 'mydet_postprocess_records_rot_nms_f32')
    assert fn(ops._ptr(tb), ops._ptr(tc), ops._ptr(ts), B, N, L['conf'], L['thr'], ctypes.byref(mode), ops._ptr(out), ops._ptr(scratch),
              ops._stream()) == 0
    torch.cuda.synchronize()
    chk_out.outside_untouched('records')
    chk_scratch.outside_untouched('scratch')
    assert chk_out.undefined_in_view() == (0, [])
    rec = ops.record_views(out.view(torch.int32).view(B, words))
    want, _ = nc.expected('N600', kind, agn)
    for i, img in enumerate(L['images']):
        _check_image(img, want[i], _host(rec, i), f'footprint {kind} {agn} {width}')


@pytest.mark.parametrize('metric', ['iou', 'ios'])
@pytest.mark.parametrize('width', [4, 5])
def test_tile_merge_agnostic(dev, metric, width):
    """mydet_merge_tile_records_nms_f32 with agnostic = 1 against the reference on the gathered candidates (hard NMS, one
    group, conf = -inf); agnostic = 0 is the shipped merge."""
    L = nc.launches()['N600']
    tb, tc, ts = _inputs(L, dev, width)
    tiles = ops.postprocess(tb, tc, ts, L['conf'], L['thr'])                      # two images = two windows of one frame
    T = 2
    origins = [(0, 0), (3, 2)]
    got = ops.merge_tile_records(tiles, 1, T, origins, L['thr'], metric, agnostic=True)
    plain = ops.merge_tile_records(tiles, 1, T, origins, L['thr'], metric)
    same = ops.merge_tile_records(tiles, 1, T, origins, L['thr'], metric, agnostic=False)
    assert torch.equal(plain['records'], same['records'])
    cand_b, cand_c, cand_s = np.zeros((T * 512, 4), np.float32), np.zeros(T * 512, np.int64), np.full(T * 512, np.nan, np.float32)
    ang = np.zeros(T * 512, np.float32)
    for t in range(T):
        h = _host(tiles, t)
        k = h['count']
        sl = slice(t * 512, t * 512 + k)
        cand_b[sl] = h['bbox'][:k, :4] + np.asarray([origins[t][0], origins[t][1], 0, 0], np.float32)
        cand_c[sl], cand_s[sl] = h['class_idx'][:k], h['score'][:k]
        if width == 5:
            ang[sl] = h['bbox'][:k, 4]
    if metric == 'ios':                                                           # the reference's pair value, swapped for this test
        want = _hard_agnostic_ios(cand_b, cand_c, cand_s, L['thr'])
    else:
        want = ref.run(cand_b, cand_c, cand_s, -np.inf, L['thr'], 'hard', agnostic=True)
    _check_image(dict(angle=ang), want, _host(got, 0), f'tile merge {metric} width {width}')
    assert want['count'] < int(plain['count'][0]), 'the agnostic merge joined nothing across classes'


def _hard_agnostic_ios(b, c, s, thr):
    """Hard agnostic NMS with intersection over the smaller area (MYDET_MERGE_IOS), float32 in the kernel's order."""
    sel, bad = ref.select(c, s, -np.inf)
    assert not bad
    sb = b[sel]
    x1, y1, x2, y2, a = ref.corners(sb)
    w = np.maximum(np.float32(0), np.minimum(x2[:, None], x2[None, :]) - np.maximum(x1[:, None], x1[None, :]))
    h = np.maximum(np.float32(0), np.minimum(y2[:, None], y2[None, :]) - np.maximum(y1[:, None], y1[None, :]))
    with np.errstate(invalid='ignore', divide='ignore'):
        o = (w * h) / np.minimum(a[:, None], a[None, :])
    kept = ref._hard(list(range(len(sel))), o, thr)
    kept.sort(key=lambda i: (int(c[sel[i]]), i))
    pos = np.asarray(kept, np.int64)
    return dict(count=len(pos), index=sel[pos].astype(np.int64), cls=c[sel[pos]], score=s[sel[pos]], bbox=sb[pos])


def test_image_objects_take_a_mode(dev):
    from mydetection_amd.utils.structures import ImageObjects
    L = nc.launches()['N65']
    img = L['images'][0]
    obj = ImageObjects(torch.from_numpy(img['b'].copy()), torch.from_numpy(img['c'].copy()), None, torch.from_numpy(img['s'].copy()), 'cxcywh',
                       img_hw=(1024, 1024))
    for kind, agn in nc.MODES:
        out = obj.post_process(L['conf'], L['thr'], nms=_nms(L, kind, agn))
        want = nc.expected('N65', kind, agn)[0][0]
        assert len(out) == want['count']
        np.testing.assert_array_equal(_bits(out.scores.cpu().numpy()), _bits(want['score']))
        np.testing.assert_array_equal(_bits(out.bboxes.cpu().numpy()), _bits(want['bbox']))
        np.testing.assert_array_equal(out.cats.cpu().numpy(), want['cls'])
    out = obj.nms(L['thr'], nms=Nms(agnostic=True))               # every box is a candidate: conf = -inf
    want = ref.run(img['b'], img['c'], img['s'], -np.inf, L['thr'], 'hard', agnostic=True)
    assert len(out) == want['count'] and np.array_equal(_bits(out.bboxes.cpu().numpy()), _bits(want['bbox']))


# ------------------------------------------------------------------------------------------------------------------ Detector level
SIZE = 64
KW = dict(preprocessing='resize_pad_square', input_size=SIZE, conf_thres=0.001)


@pytest.fixture(scope='module')
def detector(dev):
    from mydetection_amd import synth
    from mydetection_amd.api import Detector
    from mydetection_amd.models.general import name_to_model
    m, cfg = name_to_model('yolov3_80')
    m.load_state_dict(synth.make_state_dict(m.state_dict(), 'yolov3_80'), strict=True)
    return Detector(model_and_cfg=(m.eval().cuda(), cfg))


def _frames(n, h, w, seed):
    from mydetection_amd import synth
    return np.ascontiguousarray(np.stack([(synth.make_images(1, max(h, w), seed=seed + i)[0, :, :h, :w].permute(1, 2, 0).numpy() * 255)
                                          .astype(np.uint8) for i in range(n)]))


def _assert_objects_equal_records(objs, rec):
    counts = rec['count'].tolist()
    assert len(objs) == len(counts)
    for b, (o, k) in enumerate(zip(objs, counts)):
        assert len(o) == k
        assert torch.equal(o.bboxes, rec['bbox'][b, :k]) and torch.equal(o.scores, rec['score'][b, :k]) and torch.equal(o.cats, rec['class_idx'][b, :k])


def test_predict_frames_runs_the_mode_eager_and_replayed(detector):
    """predict_frames(nms=) is batched_post_process of forward_candidates with the same mode; the eager calls and the graph
    replay agree bit for bit; a call with nms=None on the same shape returns what it returned before (no shared graph)."""
    import PIL.Image
    from mydetection_amd.utils.structures import batched_post_process
    det = detector
    frames = _frames(2, SIZE, SIZE, seed=11)
    mode = Nms('soft-linear')
    before = det.predict_frames(frames, **KW)
    (idxs, x, pads, hws), = det.preprocess_batch([PIL.Image.fromarray(f) for f in frames], **KW)
    with torch.no_grad():
        bb, ci, sc = det.model.forward_candidates(x)
    want = batched_post_process(bb, ci, sc, KW['conf_thres'], det.nms_thres, nms=mode)
    plain = batched_post_process(bb, ci, sc, KW['conf_thres'], det.nms_thres)
    ops.records_to_original_(want, pads)
    assert int(want['count'].sum()) > 0 and not torch.equal(want['records'], plain['records']), 'the mode changed nothing on this input'
    runs = [det.predict_frames(frames, nms=mode, **KW) for _ in range(4)]
    for got in runs:
        _assert_objects_equal_records(got, want)
    keys = list(det._graphs.graphs)
    assert any(k[-1] == mode for k in keys), 'no graph was captured for the mode'
    for _ in range(3):                                            # by now nms=None replays its own graph
        after = det.predict_frames(frames, **KW)
        for a, b in zip(after, before):
            assert torch.equal(a.bboxes, b.bboxes) and torch.equal(a.scores, b.scores) and torch.equal(a.cats, b.cats)
    assert any(len(k) == 4 and k[0] == (2, 3, SIZE, SIZE) for k in det._graphs.graphs)
    # a second mode on the same shape is a third graph, not the first mode's
    other = Nms('soft-gaussian', sigma=0.3)
    got = [det.predict_frames(frames, nms=other, **KW) for _ in range(3)][-1]
    want2 = batched_post_process(bb, ci, sc, KW['conf_thres'], det.nms_thres, nms=other)
    ops.records_to_original_(want2, pads)
    _assert_objects_equal_records(got, want2)
    assert not torch.equal(want2['records'], want['records'])
    # the detector's own default is the same setting
    det.nms = mode
    try:
        _assert_objects_equal_records(det.predict_frames(frames, **KW), want)
        for a, b in zip(det.predict_frames(frames, nms=None, **KW), before):
            assert torch.equal(a.bboxes, b.bboxes) and torch.equal(a.scores, b.scores)
        pil = det.predict_batch([PIL.Image.fromarray(f) for f in frames], **KW)
        _assert_objects_equal_records(pil, want)
    finally:
        det.nms = None


def test_tiles_agnostic_joins_two_classes_across_a_seam(detector, monkeypatch):
    """Two windows see one object at the same frame position, one as class 0 and one as class 1.  The windows' own post-process
    cannot join them (each holds one box); the merge does with the mode's `agnostic`, and does not without."""
    from mydetection_amd.api import Tiles
    det = detector
    H, W, B = SIZE, SIZE + 32, 2
    frames = _frames(B, H, W, seed=21)
    tiles = Tiles((SIZE, SIZE), overlap=0.5, full_frame=False)                    # windows at x0 = 0 and 32: no resize, no padding
    dev = next(det.model.parameters()).device

    def forward_candidates(x):
        assert tuple(x.shape) == (2 * B, 3, SIZE, SIZE)                           # window-major
        bb = torch.zeros((2 * B, 8, 4), device=dev)
        bb[:, :, 2:] = 4
        bb[:, :, 0] = torch.arange(8, device=dev) * 6 + 3                          # filler boxes that fail conf
        ci = torch.zeros((2 * B, 8), dtype=torch.int64, device=dev)
        sc = torch.zeros((2 * B, 8), device=dev)
        bb[:B, 0] = torch.tensor([48., 30., 16., 16.], device=dev)               # frame (48, 30): window 0 sees it at x = 48
        bb[B:, 0] = torch.tensor([16., 30., 16., 16.], device=dev)               # window 1 (x0 = 32) at x = 16
        ci[B:, 0] = 1
        sc[:B, 0], sc[B:, 0] = 0.9, 0.8
        return bb, ci, sc
    monkeypatch.setattr(det.model, 'forward_candidates', forward_candidates)
    monkeypatch.setattr(det, 'use_graph', False)
    kw = dict(KW, conf_thres=0.5, tiles=tiles)
    plain = det.predict_frames(frames, **kw)
    assert [len(o) for o in plain] == [2] * B and plain[0].cats.tolist() == [0, 1]
    for mode in (Nms(agnostic=True), Nms('soft-linear', agnostic=True), Nms('merge', agnostic=True)):
        got = det.predict_frames(frames, nms=mode, **kw)
        assert [len(o) for o in got] == [1] * B, mode
        assert got[0].cats.tolist() == [0] and got[0].bboxes.tolist() == [[48., 30., 16., 16.]]
        assert got[0].scores.tolist() == [float(np.float32(0.9))]
    got = det.predict_frames(frames, nms=Nms('soft-linear'), **kw)                # not agnostic: the merge stays class-aware
    assert [len(o) for o in got] == [2] * B


def test_tracker_and_chips_take_a_mode(detector):
    from mydetection_amd.api import Chips, Tracker
    det = detector
    frames = _frames(2, SIZE, SIZE, seed=11)
    mode = Nms('soft-linear', agnostic=True)
    (idxs, rec), = det._frame_records(frames, nms=mode, **KW)
    counts = rec['count'].tolist()
    (_, plain), = det._frame_records(frames, **KW)
    assert sum(counts) > 0 and not torch.equal(rec['records'], plain['records']), 'the mode changed nothing on this input'
    objs, chips = det.crop_frames(frames, Chips((8, 8), max_per_frame=512, out='uint8'), nms=mode, **KW)
    assert [len(o) for o in objs] == counts and [len(c) for c in chips] == counts
    tracker = Tracker(streams=2, max_tracks=512, min_score=0.0)
    tracked = det.predict_frames(frames, tracker=tracker, coasting=True, nms=mode, **KW)
    print('tracked rows', [len(o) for o in tracked], 'record counts', counts)
    assert [len(o) for o in tracked] == counts
    drawn = det.annotate_frames(frames.copy(), nms=mode, **KW)
    assert [len(o) for o in drawn[0]] == counts
    rows = det.frames_to_json(frames, [1, 2], nms=mode, **KW)
    assert len(rows) == sum(counts)
