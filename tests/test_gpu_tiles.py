"""GPU tests of tiled detection on large frames: the merge of tile records (mydet_merge_tile_records_f32) against the numpy
restatement tests/_tiles_ref.py, field by field and bit for bit, at the smallest shapes that take each path; and
Detector.predict_frames / predict_frames_yuv / frames_to_json with tiles= against the same merge applied to the detections
of the window crops.

Decisions are compared exactly.  The kernel's pair values are float32, the checker's float64, so every random input comes
from a seed (fixed here, found on the CPU) for which no same-class pair of the selected candidates has a pair value within
MARGIN = 1e-5 of the threshold -- 100 x the float32 rounding of a value near 1 -- and each test asserts that.

The model-level expectation is built through the public path: predict_frames on the window crops, all crops of a call in
ONE list, so that they make the batch the tiled call makes.  (The conv dispatch of this package depends on the batch size,
so the crops of one window alone, a batch of B, do not give the bits they give inside the batch of T*B: measured on the MI355X
at the shapes below, all 10 window records of both models differ, boxes by up to 6.1e-4 px and scores by up to 5.8e-6 --
float32 round-off, profiles/tiles.md.)"""
import numpy as np
import pytest
import torch

import _tiles_ref as ref
from _arena import flat_arena

pytestmark = pytest.mark.gpu

MARGIN = 1e-5
NMS = 0.45


def _tile_fields(seed, counts, width=4, origins=None, n_cls=3, frame=(300, 400)):
    """Random window records of one frame.  counts [T] -> (boxes [T,512,width], scores [T,512], cats [T,512]) in window
    coordinates: clusters of near-duplicates around shared frame positions, so that windows see the same objects; distinct
    scores.  Slots past a window's count hold poison (a score of 2 and a box that covers everything) no merge may read."""
    rng = np.random.Generator(np.random.PCG64(seed))
    T = len(counts)
    origins = origins or [(0, 0)] * T
    K = 40
    ctr = np.stack([rng.uniform(0, frame[1], K), rng.uniform(0, frame[0], K)], 1)
    wh = rng.uniform(12, 90, size=(K, 2))
    ang = rng.uniform(-180, 180, size=K)
    kc = rng.integers(0, n_cls, size=K)
    boxes = np.empty((T, 512, width), np.float32)
    cats = np.empty((T, 512), np.int64)
    scores = rng.permutation(np.linspace(0.05, 0.95, T * 512)).astype(np.float32).reshape(T, 512)
    for t, (x0, y0) in enumerate(origins):
        k = rng.integers(0, K, size=512)
        boxes[t, :, :2] = ctr[k] + rng.normal(0, 4, size=(512, 2)) - np.array([x0, y0])
        boxes[t, :, 2:4] = wh[k] * (1 + rng.normal(0, 0.1, size=(512, 2)))
        if width == 5:
            boxes[t, :, 4] = ang[k] + rng.normal(0, 10, size=512)
        cats[t] = kc[k]
        boxes[t, max(counts[t], 0):, :4] = (0, 0, 10000, 10000)
        scores[t, max(counts[t], 0):] = 2.0
    return boxes, scores, cats


def _batch(seed, counts, width=4, origins=None):
    """B frames of T windows: (fields per frame, the [T,B,words] record buffer as numpy)."""
    frames = [_tile_fields(seed + 100 * b, c, width, origins) for b, c in enumerate(counts)]
    rec = np.stack([np.stack([ref.pack_record(f[0][t], f[1][t], f[2][t], c[t]) for f, c in zip(frames, counts)])
                    for t in range(len(counts[0]))])
    return frames, rec


def _merge(rec, origins, nms=NMS, metric='iou', rotated_nms=False, layout='tile_major'):
    """ops.merge_tile_records on a numpy [T,B,words] buffer -> the merged [B,words] buffer as numpy."""
    from mydetection_amd import ops
    T, B, words = rec.shape
    if layout == 'tile_major':
        dev = torch.from_numpy(np.ascontiguousarray(rec)).cuda().view(T * B, words)
    else:                                                            # [B][T] in memory, handed over through its strides
        dev = torch.from_numpy(np.ascontiguousarray(rec.transpose(1, 0, 2))).cuda().transpose(0, 1)
        assert dev.stride(0) == words and dev.stride(1) == T * words
    out = ops.merge_tile_records(dev, B, T, origins, nms, metric, rotated_nms)
    torch.cuda.synchronize()
    assert out['records'].shape == (B, words) and out['index'].data_ptr() == out['records'].data_ptr() + 4 * ref.REC_INDEX
    return out['records'].cpu().numpy()


def _check(got, frames, counts, origins, nms=NMS, metric='iou', rotated_nms=False, what=''):
    """Every word of the merged records equals the restatement's; returns the kept candidate lists."""
    kept_all = []
    for b, (f, c) in enumerate(zip(frames, counts)):
        kept, cb, cc, cs, order = ref.merge_frame(*f, c, origins, nms, metric, rotated_nms)
        if kept is not None:
            m = ref.margin(cb, cc, order, nms, metric, rotated_nms)
            assert m > MARGIN, f'{what}: frame {b} has a pair within {m:.2e} of the threshold; pick another seed'
        want = ref.expected_record(*f, c, origins, nms, metric, rotated_nms)
        g, w = ref.unpack_records(got[b]), ref.unpack_records(want)
        assert int(g['count']) == int(w['count']), (what, b, int(g['count']), int(w['count']))
        for name in w:
            np.testing.assert_array_equal(g[name].view(np.uint32 if g[name].dtype == np.float32 else g[name].dtype),
                                          w[name].view(np.uint32 if w[name].dtype == np.float32 else w[name].dtype),
                                          err_msg=f'{what} frame {b} field {name}')
        np.testing.assert_array_equal(got[b], want)
        kept_all.append(None if kept is None else kept.tolist())
    return kept_all


PLAIN_COUNTS = [[5, 0, 3], [512, 512, 40]]
PLAIN_ORIGINS = [(0, 0), (150, 0), (72, 54)]
PLAIN_SEED = {'iou': 2, 'ios': 2}


@pytest.mark.parametrize('layout', ['tile_major', 'frame_major'])
@pytest.mark.parametrize('metric', ['iou', 'ios'])
def test_merge_against_the_restatement(metric, layout):
    """B = 2, T = 3: frame 0 has 8 candidates in two windows (one window is empty), frame 1 has 1 064, more than 512, so the
    top-k cut runs.  Both buffer layouts give the same records."""
    frames, rec = _batch(PLAIN_SEED[metric], PLAIN_COUNTS, 4, PLAIN_ORIGINS)
    got = _merge(rec, PLAIN_ORIGINS, NMS, metric, layout=layout)
    kept = _check(got, frames, PLAIN_COUNTS, PLAIN_ORIGINS, NMS, metric, what=f'{metric} {layout}')
    assert 0 < len(kept[0]) <= 8 and 20 < len(kept[1]) < 512                     # clusters were merged, not everything
    assert {i >> 9 for i in kept[0]} <= {0, 2} and {i >> 9 for i in kept[1]} == {0, 1, 2}
    assert all((i & 511) < PLAIN_COUNTS[b][i >> 9] for b in range(2) for i in kept[b])


def _crafted(boxes0, boxes1, scores, cats, origins=((0, 0), (60, 0)), counts=(1, 1)):
    """One frame, two windows with one detection each (poison behind it)."""
    width = len(boxes0)
    b = np.zeros((2, 512, width), np.float32)
    b[:, :, 2:4] = 10000
    s = np.full((2, 512), 2.0, np.float32)
    c = np.full((2, 512), 1, np.int64)
    b[0, 0], b[1, 0] = boxes0, boxes1
    s[:, 0], c[:, 0] = scores, cats
    rec = np.stack([ref.pack_record(b[t], s[t], c[t], counts[t])[None] for t in range(2)])
    return [(b, s, c)], rec, [list(counts)], [tuple(o) for o in origins]


WHOLE, HALF = (60, 50, 40, 20), (10, 50, 20, 20)       # x 40..80 of the frame, and its part right of the seam at x = 60: IoU 0.5, IoS 1


@pytest.mark.parametrize('metric', ['iou', 'ios'])
def test_crafted_seam_pair(metric):
    thr = 0.6                                                                    # IoU 0.5 < 0.6 < IoS 1
    frames, rec, counts, origins = _crafted(WHOLE, HALF, (0.9, 0.8), (0, 0))
    got = _merge(rec, origins, thr, metric)
    kept = _check(got, frames, counts, origins, thr, metric, what='seam pair')
    assert kept[0] == ([0, 512] if metric == 'iou' else [0])                     # IoS drops the lower-scoring, truncated box
    g = ref.unpack_records(got[0])
    assert g['bbox'][0].tolist() == [60, 50, 40, 20] and (metric == 'ios' or g['bbox'][1].tolist() == [70, 50, 20, 20])
    # the higher score on the truncated box: it stays, the whole box goes
    frames, rec, counts, origins = _crafted(WHOLE, HALF, (0.7, 0.8), (0, 0))
    kept = _check(_merge(rec, origins, thr, metric), frames, counts, origins, thr, metric, what='seam pair, scores swapped')
    assert kept[0] == ([512, 0] if metric == 'iou' else [512])
    # different classes: both stay, class ascending
    frames, rec, counts, origins = _crafted(WHOLE, HALF, (0.9, 0.8), (5, 2))
    kept = _check(_merge(rec, origins, thr, metric), frames, counts, origins, thr, metric, what='seam pair, two classes')
    assert kept[0] == [512, 0]


@pytest.mark.parametrize('metric', ['iou', 'ios'])
def test_crafted_ties_zero_areas_and_bad_class(metric):
    # equal scores, one object seen by two windows: the earlier window is kept and `index` shows it
    frames, rec, counts, origins = _crafted((70, 50, 40, 20), (10, 50, 40, 20), (0.5, 0.5), (0, 0))
    got = _merge(rec, origins, NMS, metric)
    assert _check(got, frames, counts, origins, NMS, metric, what='tie')[0] == [0]
    assert ref.unpack_records(got[0])['index'][0] == 0
    frames, rec, counts, origins = _crafted((10, 50, 40, 20), (70, 50, 40, 20), (0.5, 0.5), (0, 0), origins=((60, 0), (0, 0)))
    assert _check(_merge(rec, origins, NMS, metric), frames, counts, origins, NMS, metric, what='tie, windows exchanged')[0] == [0]
    # equal scores that do not overlap: both stay, the earlier window first
    frames, rec, counts, origins = _crafted((20, 50, 10, 10), (50, 50, 10, 10), (0.5, 0.5), (0, 0))
    assert _check(_merge(rec, origins, NMS, metric), frames, counts, origins, NMS, metric, what='tie, apart')[0] == [0, 512]
    # two boxes without area on one spot: 0/0, not suppressed
    frames, rec, counts, origins = _crafted((70, 50, 0, 20), (10, 50, 0, 20), (0.9, 0.8), (0, 0))
    assert _check(_merge(rec, origins, 0.0, metric), frames, counts, origins, 0.0, metric, what='zero areas')[0] == [0, 512]
    # a window with the bad-class sentinel fails its frame
    for counts_ in ((1, -1), (-1, 1), (-1, -1)):
        frames, rec, counts, origins = _crafted(WHOLE, HALF, (0.9, 0.8), (0, 0), counts=counts_)
        got = _merge(rec, origins, NMS, metric)
        assert _check(got, frames, counts, origins, NMS, metric, what='bad class')[0] is None
        assert int(ref.unpack_records(got[0])['count']) == -1 and not got[0][1:].any()


ROT_COUNTS = [[60, 7, 0], [300, 280, 90]]
ROT_SEED = {False: 1, True: 3}


@pytest.mark.parametrize('rotated_nms', [False, True], ids=['aligned', 'rotnms'])
def test_rotated_records(rotated_nms):
    """box_width 5.  Without rotated_nms the angle travels with its box and the decisions are those of the 4-wide run on
    columns 0-3; with it the pair test is the rotated IoU with `>=` (tests/_rotbox_ref.py)."""
    frames, rec = _batch(ROT_SEED[rotated_nms], ROT_COUNTS, 5, PLAIN_ORIGINS)
    assert rec.shape[2] == ref.REC_ROT_WORDS
    got = _merge(rec, PLAIN_ORIGINS, NMS, 'iou', rotated_nms)
    kept = _check(got, frames, ROT_COUNTS, PLAIN_ORIGINS, NMS, 'iou', rotated_nms, what=f'rotated records, rotated_nms={rotated_nms}')
    assert 5 < len(kept[0]) < 67 and 20 < len(kept[1]) < 512
    g = ref.unpack_records(got)
    if not rotated_nms:
        got4 = ref.unpack_records(_merge(np.ascontiguousarray(rec[:, :, :ref.REC_WORDS]), PLAIN_ORIGINS, NMS, 'iou'))
        for name in ('count', 'bbox', 'score', 'class_idx', 'index'):
            np.testing.assert_array_equal(g[name], got4[name])
        for b in range(2):
            k = int(g['count'][b])
            idx = g['index'][b, :k]
            np.testing.assert_array_equal(g['angle'][b, :k], frames[b][0][idx >> 9, idx & 511, 4])
    else:
        aligned = ref.merge_frame(*frames[1], ROT_COUNTS[1], PLAIN_ORIGINS, NMS, 'iou', False)[0].tolist()
        assert aligned != kept[1], 'rotation decides nothing on this input: the test would show nothing'


def test_ios_with_rotated_nms_is_unsupported():
    from mydetection_amd import _lib, ops
    lib = _lib.lib()
    B, T, words = 1, 2, _lib.REC_ROT_WORDS
    rec = torch.zeros((T * B, words), dtype=torch.int32, device='cuda')
    org = torch.zeros((T, 2), dtype=torch.int32, device='cuda')
    out = torch.empty((B, words), dtype=torch.int32, device='cuda')
    nbytes = lib.mydet_merge_tile_records_scratch_bytes(B, T, 5)
    scratch = torch.empty(nbytes // 8, dtype=torch.int64, device='cuda')

    def call(metric, rot):
        return lib.mydet_merge_tile_records_f32(ops._ptr(rec), B * words, words, B, T, 5, ops._ptr(org), 0.5, metric, rot,
                                                ops._ptr(out), ops._ptr(scratch), nbytes, ops._stream())
    assert call(_lib.MERGE_IOS, 1) == -2                                         # MYDET_E_UNSUPP
    assert call(_lib.MERGE_IOS, 0) == 0 and call(_lib.MERGE_IOU, 1) == 0
    torch.cuda.synchronize()
    with pytest.raises(ValueError, match="'ios'"):
        ops.merge_tile_records(rec, B, T, [(0, 0)] * T, 0.5, metric='ios', rotated_nms=True)


@pytest.mark.parametrize('width', [4, 5])
def test_one_window_at_the_origin_returns_the_record(width):
    """T = 1, origin (0, 0), the threshold the record was made with: the merge returns its input, `index` = the slot number."""
    from mydetection_amd import ops
    rng = np.random.Generator(np.random.PCG64(3))
    B, N = 2, 700
    boxes = np.concatenate([rng.uniform(0, 300, (B, N, 2)), rng.uniform(10, 80, (B, N, 2)), rng.uniform(-180, 180, (B, N, 1))], 2)
    boxes = torch.from_numpy(boxes[:, :, :width].astype(np.float32)).cuda()
    cats = torch.from_numpy(rng.integers(0, 3, (B, N))).cuda()
    scores = torch.from_numpy(rng.random((B, N), dtype=np.float32)).cuda()
    for rotated_nms in ([False] if width == 4 else [False, True]):
        rec = ops.postprocess(boxes, cats, scores, 0.3, NMS, rotated_nms=rotated_nms)
        out = ops.merge_tile_records(rec, B, 1, [(0, 0)], NMS, rotated_nms=rotated_nms)
        torch.cuda.synchronize()
        counts = rec['count'].tolist()
        assert out['count'].tolist() == counts and min(counts) > 20
        for name in ('bbox', 'score', 'class_idx') + (('angle',) if width == 5 else ()):
            assert torch.equal(out[name], rec[name]), name
        for b, k in enumerate(counts):
            assert out['index'][b, :k].tolist() == list(range(k)) and not out['index'][b, k:].any()


@pytest.mark.parametrize('width', [4, 5])
def test_footprint(width):
    """records and scratch lie between sentinel guard bands: the bands are untouched, every word of the B records is
    written, and a scratch one byte short is refused."""
    from mydetection_amd import _lib, ops
    lib = _lib.lib()
    counts = [[512, 30, 0], [0, 0, 0]]
    B, T = 2, 3
    frames, rec = _batch(5, counts, width, PLAIN_ORIGINS)
    words = rec.shape[2]
    dev = torch.device('cuda')
    src = torch.from_numpy(rec).to(dev)
    org = torch.tensor(PLAIN_ORIGINS, dtype=torch.int32, device=dev)
    nbytes = lib.mydet_merge_tile_records_scratch_bytes(B, T, width)
    assert nbytes == B * T * 512 * (4 * width + 20)
    out, chk_out = flat_arena(B * words, dev)
    scratch, chk_scratch = flat_arena(nbytes // 4, dev)

    def call(n):
        return lib.mydet_merge_tile_records_f32(ops._ptr(src), B * words, words, B, T, width, ops._ptr(org), NMS, _lib.MERGE_IOU, 0,
                                                ops._ptr(out), ops._ptr(scratch), n, ops._stream())
    assert call(nbytes - 1) == -1
    torch.cuda.synchronize()
    assert chk_out.undefined_in_view()[0] == B * words                           # nothing was launched
    assert call(nbytes) == 0
    torch.cuda.synchronize()
    chk_out.outside_untouched('records')
    chk_scratch.outside_untouched('scratch')
    assert chk_out.undefined_in_view() == (0, [])
    got = out.view(torch.int32).view(B, words).cpu().numpy()
    _check(got, frames, counts, PLAIN_ORIGINS, NMS, 'iou', what='footprint')
    assert int(got[1, 0]) == 0 and not got[1].any()                              # a frame without detections: a record of zeros


# ---- model level ----

@pytest.fixture(scope='module', params=['yolov3_80', 'rapid'])
def detector(request):
    from mydetection_amd import synth
    from mydetection_amd.api import Detector
    from mydetection_amd.models.general import name_to_model
    name = request.param
    m, cfg = name_to_model(name)
    m.load_state_dict(synth.make_state_dict(m.state_dict(), name), strict=True)
    return name, Detector(model_and_cfg=(m.eval().cuda(), cfg))


def _synthetic_frames(n, h, w, seed):
    from mydetection_amd import synth
    return np.stack([(synth.make_images(1, max(h, w), seed=seed + i)[0, :, :h, :w].permute(1, 2, 0).numpy() * 255).astype(np.uint8)
                     for i in range(n)])


def _records_of_objects(objs, T, B):
    """The [T,B,words] record buffer (numpy) of T*B ImageObjects in window-major order."""
    recs = []
    for o in objs:
        k = len(o)
        assert k <= 512
        width = o.bboxes.shape[1]
        b, s, c = np.zeros((512, width), np.float32), np.zeros(512, np.float32), np.zeros(512, np.int64)
        b[:k], s[:k], c[:k] = o.bboxes.cpu().numpy(), o.scores.cpu().numpy(), o.cats.cpu().numpy()
        recs.append(ref.pack_record(b, s, c, k))
    return np.stack(recs).reshape(T, B, -1)


def _expected(det, crops, windows, B, nms, metric='iou', rotated_nms=False, **kw):
    """(merged record dict, window records [T,B,words]) from the detections of the window crops: the crops go through the
    public path, their detections are packed into records, shifted and merged by ops.merge_tile_records."""
    from mydetection_amd import ops
    objs = det.predict_frames(crops, rotated_nms=rotated_nms, **kw)
    T = len(windows)
    assert len(objs) == T * B and all(o.img_hw == (w[2], w[3]) for o, w in zip(objs, [w for w in windows for _ in range(B)]))
    rec = _records_of_objects(objs, T, B)
    merged = ops.merge_tile_records(torch.from_numpy(rec).cuda().view(T * B, -1), B, T, [(x0, y0) for y0, x0, _, _ in windows], nms,
                                    metric, rotated_nms)
    return merged, rec


def _assert_objects_equal_records(objs, rec, hw):
    counts = rec['count'].tolist()
    assert len(objs) == len(counts)
    for b, (o, k) in enumerate(zip(objs, counts)):
        assert o.img_hw == hw and len(o) == k
        assert torch.equal(o.bboxes[:, :4], rec['bbox'][b, :k]) and torch.equal(o.scores, rec['score'][b, :k])
        assert torch.equal(o.cats, rec['class_idx'][b, :k])
        if 'angle' in rec:
            assert o.bboxes.shape[1] == 5 and torch.equal(o.bboxes[:, 4], rec['angle'][b, :k])


H, W, B = 150, 200, 2


def test_tiled_predict_frames_equals_the_merge_of_the_crops(detector, monkeypatch):
    from mydetection_amd import ops
    from mydetection_amd.api import Tiles
    name, det = detector
    kw = dict(input_size=128, conf_thres=0.001)
    tiles = Tiles((96, 128), overlap=0.25)
    frames = torch.from_numpy(_synthetic_frames(B, H, W, seed=70)).cuda()
    windows = ops.tile_windows(H, W, (96, 128), 0.25)
    T = len(windows)
    assert T == 5 and windows[-1] == (0, 0, H, W)
    calls = []
    real = ops.merge_tile_records
    monkeypatch.setattr(ops, 'merge_tile_records', lambda *a, **k: (calls.append((a, k)), real(*a, **k))[1])
    got = det.predict_frames(frames, tiles=tiles, **kw)
    assert len(calls) == 1 and calls[0][0][1:3] == (B, T) and calls[0][0][4] == det.nms_thres
    crops = [frames[:, y0:y0 + h, x0:x0 + w] for y0, x0, h, w in windows]
    want, tile_rec = _expected(det, crops, windows, B, det.nms_thres, **kw)
    assert sum(want['count'].tolist()) > 0
    _assert_objects_equal_records(got, want, (H, W))
    # the records behind the objects: every index decodes to a detection of a window of the plan
    (idxs, rec), = det._frame_records(frames, tiles=tiles, **kw)
    assert idxs == [0, 1] and rec['img_hw'] == [(H, W)] * B
    assert torch.equal(rec['records'], want['records'])
    tile_fields = ref.unpack_records(tile_rec)
    for b, k in enumerate(rec['count'].tolist()):
        idx = rec['index'][b, :k].cpu().numpy()
        t, slot = idx >> 9, idx & 511
        assert (t < T).all() and (slot < tile_fields['count'][t, b]).all()
        shift = np.array([[windows[i][1], windows[i][0], 0, 0] for i in t], np.float32)
        np.testing.assert_array_equal(rec['bbox'][b, :k].cpu().numpy(), tile_fields['bbox'][t, b, slot] + shift)
    assert len({i >> 9 for b, k in enumerate(rec['count'].tolist()) for i in rec['index'][b, :k].tolist()}) > 1
    # by now the batch of T*B inputs has been seen three times: the last call replayed a captured graph, and gives the same bits
    assert any(k[0][0] == T * B for k in det._graphs.graphs)
    again = det.predict_frames(frames.cpu().numpy(), tiles=tiles, **kw)             # host frames this time
    _assert_objects_equal_records(again, want, (H, W))
    # json rows
    eval_type = 'cxcywhd' if name == 'rapid' else 'x1y1wh'
    rows = det.frames_to_json(frames, [7, 8], eval_type, tiles=tiles, **kw)
    assert len(rows) == sum(len(o) for o in got)
    assert rows == [r for o, i in zip(got, (7, 8)) for r in o.to_json(i, eval_type)]
    # a merge threshold and metric of its own
    calls.clear()
    got = det.predict_frames(frames, tiles=Tiles((96, 128), overlap=0.25, nms_thres=0.3, metric='ios'), **kw)
    assert calls[0][0][4:6] == (0.3, 'ios')
    want_ios, _ = _expected(det, crops, windows, B, 0.3, 'ios', **kw)
    _assert_objects_equal_records(got, want_ios, (H, W))
    assert want_ios['count'].tolist() != want['count'].tolist() or not torch.equal(want_ios['records'], want['records'])


def test_one_window_covering_the_frame_equals_the_untiled_call(detector):
    from mydetection_amd.api import Tiles
    name, det = detector
    kw = dict(input_size=128, conf_thres=0.001)
    frames = _synthetic_frames(B, H, W, seed=70)
    want = det.predict_frames(frames, **kw)
    got = det.predict_frames(frames, tiles=Tiles((256, 256), full_frame=False), **kw)
    assert sum(len(o) for o in want) > 0 and len(got) == len(want)
    for g, w in zip(got, want):
        assert g.img_hw == w.img_hw == (H, W)
        assert torch.equal(g.bboxes, w.bboxes) and torch.equal(g.scores, w.scores) and torch.equal(g.cats, w.cats)


def test_tiled_rotated_nms_uses_the_rotated_test(detector, monkeypatch):
    from mydetection_amd import ops
    from mydetection_amd.api import Tiles
    name, det = detector
    kw = dict(input_size=128, conf_thres=0.001)
    tiles = Tiles((96, 128), overlap=0.25)
    frames = torch.from_numpy(_synthetic_frames(B, H, W, seed=70)).cuda()
    if name != 'rapid':
        with pytest.raises(ValueError, match='cxcywhd'):
            det.predict_frames(frames, tiles=tiles, rotated_nms=True, **kw)
        return
    windows = ops.tile_windows(H, W, (96, 128), 0.25)
    calls = []
    real = ops.merge_tile_records
    monkeypatch.setattr(ops, 'merge_tile_records', lambda *a, **k: (calls.append((a, k)), real(*a, **k))[1])
    got = det.predict_frames(frames, tiles=tiles, rotated_nms=True, **kw)
    assert len(calls) == 1 and calls[0][0][5:7] == ('iou', True)
    crops = [frames[:, y0:y0 + h, x0:x0 + w] for y0, x0, h, w in windows]
    want, _ = _expected(det, crops, windows, B, det.nms_thres, 'iou', True, **kw)
    _assert_objects_equal_records(got, want, (H, W))
    with pytest.raises(ValueError, match="'ios'"):
        det.predict_frames(frames, tiles=Tiles((96, 128), metric='ios'), rotated_nms=True, **kw)


@pytest.mark.parametrize('layout', ['nv12', 'i420'])
def test_tiled_yuv_equals_tiled_rgb(detector, layout):
    """4:2:0 frames with tiles give what the converted RGB frames give with the same (even) windows."""
    from mydetection_amd import ops
    from mydetection_amd.api import Tiles
    name, det = detector
    kw = dict(input_size=128, conf_thres=0.001)
    rng = np.random.Generator(np.random.PCG64(9))
    h, w = 96, 128
    rgb = _synthetic_frames(B, h, w, seed=80)
    y = torch.from_numpy((rgb.astype(np.float32) @ np.array([0.257, 0.504, 0.098], np.float32) + 16).clip(0, 255).astype(np.uint8)).cuda()
    if layout == 'nv12':
        planes = (y, torch.from_numpy(rng.integers(64, 192, (B, h // 2, w // 2, 2), dtype=np.uint8)).cuda())
    else:
        planes = (y,) + tuple(torch.from_numpy(rng.integers(64, 192, (B, h // 2, w // 2), dtype=np.uint8)).cuda() for _ in range(2))
    even = Tiles((64, 96))
    even._align = 2
    assert ops.tile_windows(h, w, (64, 96), 0.2, True, 2) == [(0, 0, 64, 96), (0, 32, 64, 96), (32, 0, 64, 96), (32, 32, 64, 96), (0, 0, 96, 128)]
    want = det.predict_frames(ops.yuv420_to_rgb(planes, layout), tiles=even, **kw)
    got = det.predict_frames_yuv(planes, layout, tiles=Tiles((64, 96)), **kw)
    assert sum(len(o) for o in want) > 0 and len(got) == len(want) == B
    for g, o in zip(got, want):
        assert g.img_hw == o.img_hw == (h, w)
        assert torch.equal(g.bboxes, o.bboxes) and torch.equal(g.scores, o.scores) and torch.equal(g.cats, o.cats)
    if layout == 'nv12':
        again = det.predict_frames_nv12(planes[0], planes[1], tiles=Tiles((64, 96)), **kw)
        for g, o in zip(again, want):
            assert torch.equal(g.bboxes, o.bboxes) and torch.equal(g.scores, o.scores)
        eval_type = 'cxcywhd' if name == 'rapid' else 'x1y1wh'
        rows = det.frames_nv12_to_json(planes[0], planes[1], [3, 4], eval_type, tiles=Tiles((64, 96)), **kw)
        assert rows == [r for o, i in zip(want, (3, 4)) for r in o.to_json(i, eval_type)]
    odd = tuple(p[:, :-1] for p in planes[:1]) + tuple(planes[1:])               # 95 rows of Y, 48 of chroma: a legal odd frame
    with pytest.raises(ValueError, match='align'):
        det.predict_frames_yuv(odd, layout, tiles=Tiles((64, 96)), **kw)
