"""GPU tests of the overlay renderer (mydet_draw_boxes_rgb_u8 / mydet_draw_boxes_yuv420_u8) against the numpy restatement of
its raster rules, tests/_draw_ref.py, at the smallest shapes that take each path: 96 x 160 and 95 x 157 frames (neither a
tile multiple, the second odd), B = 2 with different counts, contiguous targets (dword stores), views with an aligned padded
pitch (dword stores with a partial last group) and crop views at odd byte offsets inside a larger buffer (byte stores) whose
every byte outside the view must stay as it was.

Axis-aligned boxes, fills, labels and every 4:2:0 sample are compared bit for bit: all box values are multiples of 1/8, so
float32 evaluates the rules exactly.  Rotated boxes are compared on every settled pixel; the unsettled ones (within 1e-3 px
of a deciding threshold, tests/_draw_ref.py) are at most 0.5 % of the painted pixels, which tests/test_draw_host.py asserts
for these same cases."""
import numpy as np
import pytest
import torch

import _draw_cases as cases
import _draw_ref as ref
from _paint_targets import KINDS, Target, _dev

pytestmark = pytest.mark.gpu

def _style(**kw):
    from mydetection_amd import ops
    return ops.draw_style(**kw)


def _draw_rgb_case(what, H, W, boxes, counts, style, scores=None, classes=None, ids=None, kinds=KINDS, settled_only=False, seed=0):
    """ops.draw_boxes on B = len(boxes) frames for every kind of target against the restatement."""
    from mydetection_amd import ops
    B = len(boxes)
    K = max(len(b) for b in boxes)
    dense = np.zeros((B, K, 5), dtype=np.float32)
    for b, rows in enumerate(boxes):
        dense[b, :len(rows)] = rows
    painted = 0
    for kind in kinds:
        tgt = Target(np.random.default_rng(seed + 1), B, H, W, 3, kind)
        before = tgt.host.copy()
        out = ops.draw_boxes(tgt.view, _dev(dense), style, counts=_dev(counts), scores=_dev(scores), classes=_dev(classes), ids=_dev(ids))
        torch.cuda.synchronize()
        assert out is tgt.view
        skip = np.zeros((B, H, W), dtype=bool)
        for b in range(B):
            skip[b] = ref.draw_rgb(tgt.host[b], dense[b], None if counts is None else counts[b], style,
                                   None if scores is None else scores[b], None if classes is None else classes[b],
                                   None if ids is None else ids[b])
        assert settled_only or not skip.any(), what
        tgt.check(f'{what} {kind}', skip if settled_only else None)
        painted += int((tgt.host != before).any(axis=-1).sum())
    return painted


@pytest.mark.parametrize('t', [1, 2, 3, 6])
def test_axis_aligned_boxes_are_bit_identical(t):
    for H, W in cases.SIZES:
        rows = cases.axis_boxes(H, W)
        classes = np.arange(2 * len(rows), dtype=np.int64).reshape(2, -1) * 5 + 1
        painted = _draw_rgb_case(f'axis t={t} {H}x{W}', H, W, [rows, rows[::-1].copy()], np.array([len(rows), 4], np.int32),
                                 _style(thickness=t, fill_alpha=128 if t == 3 else 0), classes=classes)
        assert painted > 1000
        # 4-wide rows and no counts: all K rows, angle 0
        from mydetection_amd import ops
        tgt = Target(np.random.default_rng(5), 1, H, W, 3, 'contiguous')
        ops.draw_boxes(tgt.view[0], _dev(rows[:, :4]), _style(thickness=t, color=(9, 200, 30)))
        ref.draw_rgb(tgt.host[0], rows[:, :4], None, _style(thickness=t, color=(9, 200, 30)))
        tgt.check(f'4-wide t={t}')


def test_pixels_exactly_on_a_threshold():
    """One box whose edges put pixel centres exactly on the outer, the inner and the fill threshold: <= paints, < does not."""
    from mydetection_amd import ops
    frame = torch.zeros((1, 32, 48, 3), dtype=torch.uint8, device='cuda')
    # cx 20.5, w 11, t 2: a = |j + 0.5 - 20.5| = |j - 20|; outer a <= 6.5 -> j in 14..26; hole a < 4.5 -> j in 16..24
    ops.draw_boxes(frame, torch.tensor([[[20.5, 16.0, 11.0, 9.0]]], device='cuda'), _style(thickness=2, color=(255, 255, 255)))
    # cy 16, h 9: b = |i + 0.5 - 16|; outer b <= 5.5 -> i in 11..20 (i = 10 gives 5.5: painted; i = 21 gives 5.5: painted)
    got = frame[0, :, :, 0].cpu().numpy() != 0
    want = np.zeros((32, 48), dtype=bool)
    want[10:22, 14:27] = True
    want[13:19, 16:25] = False                                       # b < 3.5 -> i + 0.5 in (12.5, 19.5) -> i in 13..18
    assert np.array_equal(got, want)
    # integer-centred box: pixel centres on the fill threshold (a == w/2 exactly) are filled
    frame.zero_()
    ops.draw_boxes(frame, torch.tensor([[[20.5, 16.5, 5.0, 3.0]]], device='cuda'), _style(thickness=1, fill_alpha=255, color=(255, 255, 255)))
    got = frame[0, :, :, 0].cpu().numpy() != 0
    want[:] = False
    want[14:19, 17:24] = True                                        # outer: a <= 3 -> j in 17..23; b <= 2 -> i in 14..18
    assert np.array_equal(got, want)


@pytest.mark.parametrize('case', cases.rotated_cases(), ids=lambda c: c[0])
def test_rotated_boxes_match_on_every_settled_pixel(case):
    name, H, W, t, alpha, frames = case
    classes = np.zeros((2, 9), dtype=np.int64)
    classes[0], classes[1, :5] = np.arange(9) * 7, np.arange(5) * 11 + 3
    painted = _draw_rgb_case(name, H, W, frames, np.array([len(f) for f in frames], np.int32), _style(thickness=t, fill_alpha=alpha),
                             classes=classes, settled_only=True)
    assert painted > 2000


def test_clipping_and_skipped_rows_and_counts():
    from mydetection_amd import ops
    for H, W in cases.SIZES:
        rows = cases.clip_skip_boxes(H, W)
        K = len(rows)
        classes = np.tile(np.arange(K, dtype=np.int64) * 3, (2, 1))
        ok = rows.copy()
        ok[np.isnan(ok) | np.isinf(ok)] = 5.0
        assert sum(ref.valid_row(r) for r in rows) == K - 5
        # frame 0: every row; frame 1: a count above K means K
        _draw_rgb_case(f'clip {H}x{W}', H, W, [rows, rows], np.array([K, 1000], np.int32), _style(thickness=3, fill_alpha=60), classes=classes,
                       settled_only=True)
        # count 0, the bad-class sentinel: the frames are left alone, whatever the rows say
        tgt = Target(np.random.default_rng(3), 2, H, W, 3, 'odd')
        ops.draw_boxes(tgt.view, _dev(np.stack([ok, ok])), _style(thickness=3, fill_alpha=60), counts=_dev(np.array([0, -1], np.int32)))
        torch.cuda.synchronize()
        tgt.check('count 0 / -1')
        # a frame whose rows are all skipped, and K = 0
        tgt = Target(np.random.default_rng(4), 1, H, W, 3, 'contiguous')
        ops.draw_boxes(tgt.view, _dev(rows[5:10][None]), _style(labels=('class',)), classes=_dev(classes[:1, 5:10]))
        ops.draw_boxes(tgt.view, torch.zeros((1, 0, 5), device='cuda'), _style())
        torch.cuda.synchronize()
        tgt.check('skipped rows')


def test_paint_order_and_fill_blending_on_overlapping_boxes():
    for n, (H, W) in enumerate(cases.SIZES):
        frames = [cases.random_boxes(40 + n, H, W, 14, False), cases.random_boxes(50 + n, H, W, 6, False)]
        classes = np.arange(28, dtype=np.int64).reshape(2, 14)
        for alpha in (100, 255, 1):
            painted = _draw_rgb_case(f'overlap a={alpha}', H, W, frames, np.array([14, 6], np.int32), _style(thickness=2, fill_alpha=alpha),
                                     classes=classes, kinds=('contiguous', 'odd'))
            assert painted > 0.5 * H * W                             # the boxes overlap: order and repeated blending decide most pixels


def test_labels_at_the_frame_edges_and_wider_than_the_frame():
    names = ['person', 'a-rather-long-class-name', 'x', '']
    for H, W in cases.SIZES:
        rows = cases.label_boxes(H, W)
        K = len(rows)
        classes = np.stack([np.arange(K, dtype=np.int64) % 5, np.arange(K, dtype=np.int64)[::-1] * 3])
        scores = np.linspace(0.05, 0.995, 2 * K).astype(np.float32).reshape(2, K)
        ids = np.array([[1, 22, 333, 10 ** 10 + 7, -1, 98765], [5, 6, 7, 8, 9, 12345678901234]], dtype=np.int64)
        for labels, class_names, height in ((('class', 'score'), None, 10), (('class', 'score', 'id'), names, 8), (('id',), None, 16),
                                            (('score', 'class', 'id'), names, 16)):
            st = _style(thickness=2, labels=labels, label_height=height, class_names=class_names, color_by='id' if labels == ('id',) else 'class')
            _draw_rgb_case(f'labels {labels} {height}', H, W, [rows, rows], np.array([K, K - 1], np.int32), st, scores=scores, classes=classes, ids=ids,
                           settled_only=True)
        # wider than the frame: 16 + 5 + 12 glyphs of 16 columns
        st = _style(labels=('class', 'score', 'id'), label_height=16, class_names=['w' * 16])
        from mydetection_amd import ops
        assert len(ops.draw_label_text(0, 1.0, 9999999999, ['w' * 16])) * ops.glyph_atlas(16).shape[2] > W
        _draw_rgb_case('wide label', H, W, [rows[4:5]], None, st, scores=np.ones((1, 1), np.float32), classes=np.zeros((1, 1), np.int64),
                       ids=np.full((1, 1), 9999999999, np.int64))


def _records(rng, B, H, W, counts, rotated):
    """A full record buffer (numpy int32 [B, words]) of small boxes at multiples of 1/8, and its fields."""
    from mydetection_amd import _lib
    words = _lib.REC_ROT_WORDS if rotated else _lib.REC_WORDS
    rec = np.zeros((B, words), dtype=np.int32)
    boxes = np.zeros((B, 512, 5), dtype=np.float32)
    boxes[..., 0], boxes[..., 1] = cases.eighths(rng, 0, W, (B, 512)), cases.eighths(rng, 0, H, (B, 512))
    boxes[..., 2], boxes[..., 3] = cases.eighths(rng, 2, 24, (B, 512)), cases.eighths(rng, 2, 24, (B, 512))
    if rotated:
        boxes[..., 4] = rng.uniform(-180, 180, size=(B, 512))
    scores = rng.uniform(0, 1, size=(B, 512)).astype(np.float32)
    classes = rng.integers(0, 80, size=(B, 512)).astype(np.int64)
    rec[:, _lib.REC_COUNT] = counts
    rec[:, _lib.REC_BBOX:_lib.REC_SCORE] = boxes[..., :4].reshape(B, -1).view(np.int32)
    rec[:, _lib.REC_SCORE:_lib.REC_CLASS] = scores.view(np.int32)
    rec[:, _lib.REC_CLASS:_lib.REC_INDEX] = classes.view(np.int32).reshape(B, -1)
    if rotated:
        rec[:, _lib.REC_ANGLE:] = boxes[..., 4].view(np.int32)
    return rec, boxes, scores, classes


@pytest.mark.parametrize('rotated', [False, True])
def test_draw_records_reads_a_full_record_buffer_in_place(rotated):
    from mydetection_amd import ops
    H, W = cases.SIZES[1]
    counts = np.array([512, 300], np.int32)
    rec, boxes, scores, classes = _records(np.random.default_rng(7 + rotated), 2, H, W, counts, rotated)
    dev = ops.record_views(torch.from_numpy(rec).cuda())
    st = _style(thickness=1, fill_alpha=40, labels=('class', 'score'), label_height=8)
    for kind in ('contiguous', 'odd'):
        tgt = Target(np.random.default_rng(9), 2, H, W, 3, kind)
        assert ops.draw_records(tgt.view, dev, st) is tgt.view
        torch.cuda.synchronize()
        skip = np.stack([ref.draw_rgb(tgt.host[b], boxes[b] if rotated else boxes[b, :, :4], counts[b], st, scores[b], classes[b]) for b in range(2)])
        assert rotated or not skip.any()
        tgt.check(f'records rotated={rotated} {kind}', skip)
    assert torch.equal(dev['records'].cpu(), torch.from_numpy(rec))   # read only
    with pytest.raises(ValueError, match='copies'):
        ops.draw_records(tgt.view, {k: v.clone() for k, v in dev.items()}, st)
    # more than 512 dense rows go in chunks that keep the paint order
    if not rotated:
        K = 700
        many = np.concatenate([boxes[0], boxes[1]])[:K, :4]
        cls = np.concatenate([classes[0], classes[1]])[:K]
        st = _style(thickness=2, fill_alpha=90)
        for cnt in (None, np.array([600], np.int32)):
            tgt = Target(np.random.default_rng(10), 1, H, W, 3, 'pitched')
            ops.draw_boxes(tgt.view, _dev(many[None]), st, counts=_dev(cnt), classes=_dev(cls[None]))
            torch.cuda.synchronize()
            ref.draw_rgb(tgt.host[0], many, None if cnt is None else cnt[0], st, None, cls)
            tgt.check(f'chunks {cnt}')


@pytest.mark.parametrize('layout', ['nv12', 'nv21', 'i420', 'yv12'])
def test_every_8bit_420_layout_equals_the_restatement(layout):
    from mydetection_amd import ops
    planar = layout in ('i420', 'yv12')
    names = ['person', 'bicycle']
    for (H, W), kinds in ((cases.SIZES[1], KINDS), (cases.SIZES[0], ('contiguous', 'odd'))):
        H2, W2 = (H + 1) // 2, (W + 1) // 2
        rows = np.concatenate([cases.axis_boxes(H, W)[:5], cases.label_boxes(H, W)[:5], cases.clip_skip_boxes(H, W)[:4]])
        rows[:, 4] = 0
        K = len(rows)
        classes = np.stack([np.arange(K, dtype=np.int64), np.arange(K, dtype=np.int64)[::-1] * 2])
        scores = np.linspace(0.01, 0.99, 2 * K).astype(np.float32).reshape(2, K)
        counts = np.array([K, 9], np.int32)
        for kind in kinds:
            for (matrix, full), st in ((('bt601', False), _style(thickness=2, fill_alpha=77, labels=('class', 'score'), label_height=9, class_names=names)),
                                       (('bt709', True), _style(thickness=3, labels=('score',), label_height=12))):
                rng = np.random.default_rng(21)
                ty = Target(rng, 2, H, W, 0, kind)
                tc = [Target(rng, 2, H2, W2, 0, kind) for _ in range(2)] if planar else [Target(rng, 2, H2, W2, 2, kind)]
                planes = (ty.view,) + tuple(t.view for t in tc)
                out = ops.draw_boxes_yuv420(planes, layout, _dev(np.stack([rows, rows])), st, counts=_dev(counts), scores=_dev(scores),
                                            classes=_dev(classes), matrix=matrix, full_range=full)
                torch.cuda.synchronize()
                assert out is planes
                for b in range(2):
                    if planar:
                        u, v = (tc[0].host[b], tc[1].host[b]) if layout == 'i420' else (tc[1].host[b], tc[0].host[b])
                    else:
                        u, v = (tc[0].host[b, :, :, 0], tc[0].host[b, :, :, 1]) if layout == 'nv12' else (tc[0].host[b, :, :, 1], tc[0].host[b, :, :, 0])
                    uns = ref.draw_yuv(ty.host[b], u, v, rows, counts[b], st, matrix, full, scores[b], classes[b])
                    assert not uns.any()
                what = f'{layout} {H}x{W} {kind} {matrix} {full}'
                ty.check(what + ' Y')
                for t in tc:
                    t.check(what + ' chroma')
    with pytest.raises(ValueError, match='p010'):
        ops.draw_boxes_yuv420((torch.zeros((1, 8, 8), dtype=torch.int16, device='cuda'), torch.zeros((1, 4, 4, 2), dtype=torch.int16, device='cuda')),
                              'p010', torch.zeros((1, 1, 4), device='cuda'), _style())


@pytest.fixture(scope='module')
def detector():
    from mydetection_amd import synth
    from mydetection_amd.api import Detector
    from mydetection_amd.models.general import name_to_model
    m, cfg = name_to_model('rapid')
    m.load_state_dict(synth.make_state_dict(m.state_dict(), 'rapid'), strict=True)
    return Detector(model_and_cfg=(m.eval().cuda(), cfg))


def _frames(n, h, w, seed):
    from mydetection_amd import synth
    return np.ascontiguousarray(np.stack([(synth.make_images(1, max(h, w), seed=seed + i)[0, :, :h, :w].permute(1, 2, 0).numpy() * 255).astype(np.uint8)
                                          for i in range(n)]))         # packed pixels: a device tensor of them is drawn in place


def _same_objects(a, b):
    assert len(a) == len(b)
    for o, p in zip(a, b):
        assert torch.equal(o.bboxes, p.bboxes) and torch.equal(o.scores, p.scores) and torch.equal(o.cats, p.cats) and o.img_hw == p.img_hw
        assert (o.obj_ids is None) == (p.obj_ids is None) and (o.obj_ids is None or torch.equal(o.obj_ids, p.obj_ids))


def _drawn_from_objects(frames, objs, style):
    """ops.draw_boxes of a list of ImageObjects on a device copy of the frames."""
    from mydetection_amd import ops
    from mydetection_amd.utils.visualization import objects_to_rows
    out = torch.from_numpy(frames).cuda()
    boxes, counts, scores, classes, ids = objects_to_rows(objs, out.device)
    return ops.draw_boxes(out, boxes, style, counts=counts, scores=scores, classes=classes, ids=ids)


def test_annotate_frames_returns_the_objects_of_predict_frames_and_draws_them(detector):
    from mydetection_amd.api import Draw, Tiles
    det = detector
    H, W, B = 150, 200, 2
    kw = dict(input_size=128, conf_thres=0.001)
    frames = _frames(B, H, W, seed=90)
    for extra in ({}, {'tiles': Tiles((96, 128), overlap=0.25)}):
        draw = Draw(labels=('class', 'score'), label_height=8, fill_alpha=50)
        want = det.predict_frames(frames, **kw, **extra)
        assert sum(len(o) for o in want) > 0
        dev_in = torch.from_numpy(frames).cuda()
        objs, drawn = det.annotate_frames(dev_in, draw, **kw, **extra)
        _same_objects(objs, want)
        assert drawn.data_ptr() == dev_in.data_ptr()                 # a single device tensor is drawn in place
        expect = _drawn_from_objects(frames, want, draw.style((H, W)))
        assert torch.equal(drawn, expect) and not torch.equal(drawn.cpu(), torch.from_numpy(frames))
        objs2, drawn2 = det.annotate_frames(list(frames), draw, **kw, **extra)       # host frames: the batch the call built
        _same_objects(objs2, want)
        assert drawn2.is_cuda and torch.equal(drawn2, expect)
    # no detections: the frames come back bit-identical
    objs, drawn = det.annotate_frames(frames, Draw(fill_alpha=200), input_size=128, conf_thres=2.0)
    assert all(len(o) == 0 for o in objs) and torch.equal(drawn.cpu(), torch.from_numpy(frames))


def test_annotate_frames_with_a_tracker_shows_ids_and_keeps_colours(detector):
    from mydetection_amd import ops
    from mydetection_amd.api import Draw, Tracker
    det = detector
    H, W = 150, 200
    kw = dict(input_size=128, conf_thres=0.001)
    base = _frames(1, H, W, seed=90)[0]
    frames = np.stack([base, base])
    draw = Draw(labels=('class', 'score', 'id'), label_height=8)
    trk, trk_ref = Tracker(min_score=0.0005), Tracker(min_score=0.0005)
    seen = {}
    for call in range(2):
        want = det.predict_frames(frames, tracker=trk_ref, **kw)
        objs, drawn = det.annotate_frames(frames, draw, tracker=trk, **kw)
        _same_objects(objs, want)
        style = draw.style((H, W), tracked=True)
        assert style.color_mode == ops.DRAW_COLOR_MODES['id'] and style.label_flags == 7
        assert torch.equal(drawn, _drawn_from_objects(frames, want, style))
        pal = ops.draw_palette(style.n_palette)
        for o in objs:
            for i in o.obj_ids.tolist():                             # the colour is a function of the id alone: stable across calls
                assert seen.setdefault(i, tuple(pal[i % style.n_palette])) == tuple(pal[i % style.n_palette])
    assert seen and set(objs[0].obj_ids.tolist()) & set(objs[1].obj_ids.tolist())
    # the id part is in the label: drawing the same tracks without ids gives other pixels
    no_id = _drawn_from_objects(frames, want, ops.draw_style(thickness=style.thickness, color_by='id', labels=('class', 'score'), label_height=8))
    assert not torch.equal(no_id, drawn)


def test_annotate_frames_nv12_and_detect_one_return_img(detector):
    import PIL.Image
    from mydetection_amd import ops
    from mydetection_amd.api import Draw
    from mydetection_amd.utils.visualization import objects_to_rows
    det = detector
    H, W, B = 150, 200, 2
    kw = dict(input_size=128, conf_thres=0.001)
    frames = _frames(B, H, W, seed=90)
    y = np.ascontiguousarray(frames[:, :, :, 0])
    uv = np.full((B, H // 2, W // 2, 2), 128, np.uint8)
    draw = Draw(labels=('class', 'score'), label_height=8)
    want = det.predict_frames_nv12(y, uv, **kw)
    assert sum(len(o) for o in want) > 0
    yd, uvd = torch.from_numpy(y).cuda(), torch.from_numpy(uv).cuda()
    objs, drawn = det.annotate_frames_nv12(yd, uvd, draw, **kw)
    _same_objects(objs, want)
    assert drawn[0].data_ptr() == yd.data_ptr() and drawn[1].data_ptr() == uvd.data_ptr()
    ey, euv = torch.from_numpy(y).cuda(), torch.from_numpy(uv).cuda()
    boxes, counts, scores, classes, ids = objects_to_rows(want, ey.device)
    ops.draw_boxes_yuv420((ey, euv), 'nv12', boxes, draw.style((H, W)), counts=counts, scores=scores, classes=classes)
    assert torch.equal(yd, ey) and torch.equal(uvd, euv) and not torch.equal(yd.cpu(), torch.from_numpy(y))
    # one surface [B, H*3/2, W]: drawn in place, the same planes
    surface = torch.cat([torch.from_numpy(y), torch.from_numpy(uv).reshape(B, H // 2, W)], dim=1).cuda()
    objs, drawn = det.annotate_frames_nv12(surface, None, draw, **kw)
    _same_objects(objs, want)
    assert drawn.data_ptr() == surface.data_ptr() and torch.equal(surface[:, :H], ey) and torch.equal(surface[:, H:].reshape(B, H // 2, W // 2, 2), euv)
    with pytest.raises(ValueError, match='p010'):
        det.annotate_frames_yuv((y.astype(np.uint16), uv.astype(np.uint16)), 'p010', draw, **kw)
    # detect_one(return_img=True): the annotated numpy image, as the reference returns it
    img = PIL.Image.fromarray(frames[0])
    dts = det.detect_one(pil_img=img, **kw)
    np_img = det.detect_one(pil_img=img, return_img=True, line_width=2, **kw)
    assert isinstance(np_img, np.ndarray) and np_img.shape == (H, W, 3) and np_img.dtype == np.uint8 and len(dts) > 0
    expect = frames[0].copy()
    assert dts.draw_on_np(expect, line_width=2) is expect
    assert np.array_equal(np_img, expect) and not np.array_equal(np_img, frames[0])
    st = ops.draw_style(thickness=2, labels=('class', 'score'), label_height=10)
    assert np.array_equal(np_img, _drawn_from_objects(frames[:1], [dts], st)[0].cpu().numpy())
    with pytest.raises(NotImplementedError):
        det.detect_one(pil_img=img, show_img=True, **kw)


def test_annotate_and_crop_launch_what_predict_launches_plus_one(detector):
    """What the docstrings of annotate_frames* and crop_frames* promise, in the launch counts of an ops.KernelTimer: each call
    is its predict_frames* call plus ONE 'draw_boxes' / 'crop_boxes' launch -- RGB and NV12; plain, tiled and tracked -- and
    the tracked predict_frames* is the untracked one plus ONE 'track_frames'."""
    from mydetection_amd import ops
    from mydetection_amd.api import Tiles, Tracker
    det = detector
    kw = dict(input_size=128, conf_thres=0.001)
    frames = _frames(2, 150, 200, seed=90)
    y, uv = np.ascontiguousarray(frames[:, :, :, 0]), np.full((2, 75, 100, 2), 128, np.uint8)

    def launches(method, *args, **extra):
        ops.TIMER = ops.KernelTimer()
        method(*args, **kw, **extra)
        torch.cuda.synchronize()
        return {name: n for name, (n, _, _) in ops.TIMER.summary().items()}

    def plus(counts, name):
        assert name not in counts
        return dict(counts, **{name: 1})

    modes = {'plain': dict, 'tiled': lambda: {'tiles': Tiles((96, 128), overlap=0.25)},
             'tracked': lambda: {'tracker': Tracker(min_score=0.0005)}}     # synthetic weights: keep the low scores alive
    graph, timer = det.use_graph, ops.TIMER
    det.use_graph = False
    try:
        predicted = {}
        for mode, extra in modes.items():
            rgb = predicted[mode, 'rgb'] = launches(det.predict_frames, frames, **extra())
            assert launches(det.annotate_frames, frames, **extra()) == plus(rgb, 'draw_boxes'), mode
            assert launches(det.crop_frames, frames, **extra()) == plus(rgb, 'crop_boxes'), mode
            nv12 = predicted[mode, 'nv12'] = launches(det.predict_frames_nv12, y, uv, **extra())
            assert launches(det.annotate_frames_nv12, y, uv, **extra()) == plus(nv12, 'draw_boxes'), mode
            assert launches(det.crop_frames_nv12, y, uv, **extra()) == plus(nv12, 'crop_boxes'), mode
        for fmt in ('rgb', 'nv12'):
            assert predicted['tracked', fmt] == plus(predicted['plain', fmt], 'track_frames')
            assert predicted['tiled', fmt]['merge_tile_records'] == 1 and 'merge_tile_records' not in predicted['plain', fmt]
    finally:
        det.use_graph, ops.TIMER = graph, timer
