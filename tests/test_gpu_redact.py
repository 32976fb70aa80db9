"""GPU tests of the redaction (mydet_redact_boxes_rgb_u8 / mydet_redact_boxes_yuv420_u8) against the numpy restatement of its
rules, tests/_redact_ref.py, at the smallest shapes that take each path: 96 x 160 and 95 x 157 frames (neither a tile multiple,
the second odd), B = 2 with different counts, contiguous targets (dword accesses), views with an aligned padded pitch (dword
accesses with a partial last group) and crop views at odd byte offsets inside a larger buffer (byte accesses) whose every byte
outside the view must stay as it was.

Axis-aligned boxes and every 4:2:0 sample are compared bit for bit: all box values are multiples of 1/8 and pad is 1.0 or
1.25, so float32 evaluates the coverage exactly.  Rotated rows and ellipses are compared on every settled pixel; the unsettled
ones (within 1e-3 px of the deciding threshold, tests/_redact_ref.py) are at most 0.5 % of the covered pixels, which
tests/test_redact_host.py asserts for these same lists."""
import numpy as np
import pytest
import torch

import _draw_cases as cases
import _redact_ref as ref
from _paint_targets import KINDS, Target, _dev

pytestmark = pytest.mark.gpu

MODES = ('mosaic', 'smooth', 'solid')


def _style(*args, **kw):
    from mydetection_amd import ops
    return ops.redact_style(*args, **kw)


def _dense(boxes):
    B, K = len(boxes), max(len(b) for b in boxes)
    dense = np.zeros((B, K, 5), dtype=np.float32)
    for b, rows in enumerate(boxes):
        dense[b, :len(rows)] = rows
    return dense


def _rgb_case(what, H, W, boxes, counts, style, classes=None, kinds=KINDS, settled_only=False, seed=0):
    """ops.redact_boxes on B = len(boxes) frames for every kind of target against the restatement; returns the pixels changed."""
    from mydetection_amd import ops
    B, dense = len(boxes), _dense(boxes)
    changed = 0
    for kind in kinds:
        tgt = Target(np.random.default_rng(seed + 1), B, H, W, 3, kind)
        before = tgt.host.copy()
        out = ops.redact_boxes(tgt.view, _dev(dense), style, counts=_dev(counts), classes=_dev(classes))
        torch.cuda.synchronize()
        assert out is tgt.view
        skip = np.stack([ref.redact_rgb(tgt.host[b], dense[b], None if counts is None else counts[b], style,
                                        None if classes is None else classes[b]) for b in range(B)])
        assert settled_only or not skip.any(), what
        tgt.check(f'{what} {kind}', skip if settled_only else None)
        changed += int((tgt.host != before).any(axis=-1).sum())
    return changed


@pytest.mark.parametrize('cell', [4, 6, 16, 64])
@pytest.mark.parametrize('mode', MODES)
def test_axis_aligned_boxes_are_bit_identical(mode, cell):
    for H, W in cases.SIZES:
        rows = cases.axis_boxes(H, W)
        for pad in (1.0, 1.25):
            changed = _rgb_case(f'axis {mode} c={cell} pad={pad} {H}x{W}', H, W, [rows, rows[::-1].copy()], np.array([len(rows), 4], np.int32),
                                _style(mode, cell, pad=pad, color=(200, 30, 9)))
            assert changed > 3000
    # 4-wide rows, one frame and no counts: all K rows, angle 0
    from mydetection_amd import ops
    tgt = Target(np.random.default_rng(5), 1, H, W, 3, 'contiguous')
    ops.redact_boxes(tgt.view[0], _dev(rows[:, :4]), _style(mode, cell))
    ref.redact_rgb(tgt.host[0], rows[:, :4], None, _style(mode, cell))
    tgt.check(f'4-wide {mode} c={cell}')


@pytest.mark.parametrize('case', cases.rotated_cases(), ids=lambda c: c[0])
def test_rotated_rows_and_ellipses_match_on_every_settled_pixel(case):
    name, H, W, t, _, frames = case
    counts = np.array([len(f) for f in frames], np.int32)
    n = 0
    for shape in ('box', 'ellipse'):
        for pad in (1.0, 1.25):
            mode, cell = MODES[n % 3], (6, 16, 4, 64)[n % 4]
            n += 1
            changed = _rgb_case(f'{name} {shape} {pad} {mode} c={cell}', H, W, frames, counts, _style(mode, cell, shape, pad, color=(1, 2, 3)),
                                settled_only=True, kinds=('contiguous', 'odd') if t == 3 else KINDS)
            assert changed > 2000


@pytest.mark.parametrize('mode', MODES)
def test_axis_aligned_ellipses_match_on_every_settled_pixel(mode):
    for H, W in cases.SIZES:
        rows = cases.axis_boxes(H, W)
        for pad in (1.0, 1.25):
            _rgb_case(f'ellipse {mode} {pad}', H, W, [rows, rows[:3]], None, _style(mode, 6, 'ellipse', pad, color=(0, 255, 0)), settled_only=True)


def test_clipping_and_skipped_rows_and_counts():
    from mydetection_amd import ops
    for H, W in cases.SIZES:
        rows = cases.clip_skip_boxes(H, W)
        K = len(rows)
        ok = rows.copy()
        ok[np.isnan(ok) | np.isinf(ok)] = 5.0
        assert sum(ref.valid_row(r) for r in rows) == K - 5
        for mode in MODES:
            # frame 0: every row; frame 1: a count above K means K
            _rgb_case(f'clip {mode} {H}x{W}', H, W, [rows, rows], np.array([K, 1000], np.int32), _style(mode, 16, pad=1.25), settled_only=True)
            # count 0, the bad-class sentinel: the frames are left alone, whatever the rows say
            tgt = Target(np.random.default_rng(3), 2, H, W, 3, 'odd')
            ops.redact_boxes(tgt.view, _dev(np.stack([ok, ok])), _style(mode, 4), counts=_dev(np.array([0, -1], np.int32)))
            torch.cuda.synchronize()
            tgt.check('count 0 / -1')
            # a frame whose rows are all skipped, and K = 0
            tgt = Target(np.random.default_rng(4), 1, H, W, 3, 'contiguous')
            ops.redact_boxes(tgt.view, _dev(rows[5:10][None]), _style(mode, 4))
            ops.redact_boxes(tgt.view, torch.zeros((1, 0, 5), device='cuda'), _style(mode, 4))
            torch.cuda.synchronize()
            tgt.check('skipped rows')


def test_a_class_filter_leaves_the_other_classes_untouched():
    from mydetection_amd import ops
    for H, W in cases.SIZES:
        frames = [cases.random_boxes(40, H, W, 14, False), cases.random_boxes(50, H, W, 6, False)]
        classes = np.arange(28, dtype=np.int64).reshape(2, 14) % 5
        for mode in MODES:
            st = _style(mode, 6, classes=[1, 3], color=(255, 0, 255))
            changed = _rgb_case(f'filter {mode}', H, W, frames, np.array([14, 6], np.int32), st, classes=classes, kinds=('contiguous', 'odd'))
            assert changed > 500
        # the same pixels as redacting the rows of those classes alone
        tgt, alone = (Target(np.random.default_rng(8), 1, H, W, 3, 'contiguous') for _ in range(2))
        keep = np.isin(classes[0], [1, 3])
        ops.redact_boxes(tgt.view, _dev(frames[0][None]), st, classes=_dev(classes[:1]))
        ops.redact_boxes(alone.view, _dev(frames[0][keep][None]), _style('solid', 6, color=(255, 0, 255)))
        assert torch.equal(tgt.flat, alone.flat)
        with pytest.raises(ValueError, match='class filter'):
            ops.redact_boxes(tgt.view, _dev(frames[0][None]), st)


def test_whole_frame_smooth_coverage_reads_no_repainted_cell():
    """One row covers the whole of a frame of several tiles both ways: every cell is repainted by some workgroup while its
    neighbours' pixels interpolate it -- the case an in-place read of a neighbour's repainted cell would break."""
    from mydetection_amd import ops
    H, W = 160, 256
    rows = np.concatenate([np.array([[W / 2, H / 2, 2.0 * W, 2.0 * H, 0]], np.float32), cases.axis_boxes(H, W)])
    outs = []
    for order in (rows, rows[::-1].copy()):
        for kind in ('contiguous', 'odd'):
            tgt = Target(np.random.default_rng(11), 2, H, W, 3, kind)
            before = tgt.host.copy()
            ops.redact_boxes(tgt.view, _dev(np.stack([order, order])), _style('smooth', 16), counts=_dev(np.array([len(rows), 1 if order is rows else len(rows)], np.int32)))
            torch.cuda.synchronize()
            for b in range(2):
                assert not ref.redact_rgb(tgt.host[b], rows[:1], None, _style('smooth', 16)).any()
            tgt.check(f'whole frame {kind}')
            assert (tgt.host != before).any(axis=-1).mean() > 0.9
            outs.append(tgt.view.cpu())
    assert torch.equal(outs[0], outs[2]) and torch.equal(outs[1], outs[3])      # the reversed list: the same bytes


def _yuv_targets(rng, layout, B, H, W, kind):
    planar = layout in ('i420', 'yv12')
    H2, W2 = (H + 1) // 2, (W + 1) // 2
    ty = Target(rng, B, H, W, 0, kind)
    tc = [Target(rng, B, H2, W2, 0, kind) for _ in range(2)] if planar else [Target(rng, B, H2, W2, 2, kind)]
    return ty, tc


def _uv_of(layout, tc, b):
    if layout in ('i420', 'yv12'):
        return (tc[0].host[b], tc[1].host[b]) if layout == 'i420' else (tc[1].host[b], tc[0].host[b])
    return (tc[0].host[b, :, :, 0], tc[0].host[b, :, :, 1]) if layout == 'nv12' else (tc[0].host[b, :, :, 1], tc[0].host[b, :, :, 0])


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('layout', ['nv12', 'nv21', 'i420', 'yv12'])
def test_every_8bit_420_layout_equals_the_restatement(layout, mode):
    from mydetection_amd import ops
    for (H, W), kinds in ((cases.SIZES[1], KINDS), (cases.SIZES[0], ('contiguous', 'odd'))):
        rows = np.concatenate([cases.axis_boxes(H, W), cases.clip_skip_boxes(H, W)[:4], np.array([[W - 0.5, H - 0.5, 1.0, 1.0, 0]], np.float32)])
        rows[:, 4] = 0
        K = len(rows)
        counts = np.array([K, 9], np.int32)
        for kind in kinds:
            for (matrix, full), cell, pad in ((('bt601', False), 6, 1.0), (('bt709', True), 16, 1.25), (('bt709', False), 4, 1.0), (('bt601', True), 64, 1.25)):
                st = _style(mode, cell, pad=pad, color=(250, 128, 3))
                ty, tc = _yuv_targets(np.random.default_rng(21), layout, 2, H, W, kind)
                planes = (ty.view,) + tuple(t.view for t in tc)
                out = ops.redact_boxes_yuv420(planes, layout, _dev(np.stack([rows, rows])), st, counts=_dev(counts), matrix=matrix, full_range=full)
                torch.cuda.synchronize()
                assert out is planes
                for b in range(2):
                    u, v = _uv_of(layout, tc, b)
                    uns, unc = ref.redact_yuv(ty.host[b], u, v, rows, counts[b], st, matrix, full)
                    assert not uns.any() and not unc.any()
                what = f'{layout} {mode} {H}x{W} {kind} {matrix} {full} c={cell}'
                ty.check(what + ' Y')
                for t in tc:
                    t.check(what + ' chroma')
    with pytest.raises(ValueError, match='p010'):
        ops.redact_boxes_yuv420((torch.zeros((1, 8, 8), dtype=torch.int16, device='cuda'), torch.zeros((1, 4, 4, 2), dtype=torch.int16, device='cuda')),
                                'p010', torch.zeros((1, 1, 4), device='cuda'), _style())


def test_rotated_ellipses_in_nv12_match_on_every_settled_sample():
    from mydetection_amd import ops
    name, H, W, _, _, frames = cases.rotated_cases()[4]
    dense, counts = _dense(frames), np.array([len(f) for f in frames], np.int32)
    for mode in MODES:
        st = _style(mode, 6, 'ellipse', 1.25, color=(9, 99, 199))
        ty, tc = _yuv_targets(np.random.default_rng(31), 'nv12', 2, H, W, 'odd')
        ops.redact_boxes_yuv420((ty.view, tc[0].view), 'nv12', _dev(dense), st, counts=_dev(counts))
        torch.cuda.synchronize()
        skips = [ref.redact_yuv(ty.host[b], *_uv_of('nv12', tc, b), dense[b], counts[b], st) for b in range(2)]
        ty.check(f'{name} {mode} Y', np.stack([s[0] for s in skips]))
        tc[0].check(f'{name} {mode} UV', np.stack([s[1] for s in skips]))


def _records(rng, B, H, W, counts, rotated):
    """A full record buffer (numpy int32 [B, words]) of small boxes at multiples of 1/8, and its fields."""
    from mydetection_amd import _lib
    words = _lib.REC_ROT_WORDS if rotated else _lib.REC_WORDS
    rec = np.zeros((B, words), dtype=np.int32)
    boxes = np.zeros((B, 512, 5), dtype=np.float32)
    boxes[..., 0], boxes[..., 1] = cases.eighths(rng, 0, W, (B, 512)), cases.eighths(rng, 0, H, (B, 512))
    boxes[..., 2], boxes[..., 3] = cases.eighths(rng, 1, 8, (B, 512)), cases.eighths(rng, 1, 8, (B, 512))
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
    return rec, boxes, classes


@pytest.mark.parametrize('rotated', [False, True])
def test_redact_records_reads_a_full_record_buffer_in_place(rotated):
    from mydetection_amd import ops
    H, W = cases.SIZES[1]
    counts = np.array([512, 300], np.int32)
    rec, boxes, classes = _records(np.random.default_rng(7 + rotated), 2, H, W, counts, rotated)
    dev = ops.record_views(torch.from_numpy(rec).cuda())
    for st in (_style('smooth', 6), _style('mosaic', 4, classes=list(range(0, 80, 5)))):
        for kind in ('contiguous', 'odd'):
            tgt = Target(np.random.default_rng(9), 2, H, W, 3, kind)
            before = tgt.host.copy()
            assert ops.redact_records(tgt.view, dev, st) is tgt.view
            torch.cuda.synchronize()
            skip = np.stack([ref.redact_rgb(tgt.host[b], boxes[b] if rotated else boxes[b, :, :4], counts[b], st, classes[b]) for b in range(2)])
            assert rotated or not skip.any()
            tgt.check(f'records rotated={rotated} {kind}', skip)
            share = (tgt.host != before).any(axis=-1).mean()
            assert 0.03 < share < 0.95                                # some tiles and cells are reached, some pixels are not covered
    assert torch.equal(dev['records'].cpu(), torch.from_numpy(rec))   # read only
    with pytest.raises(ValueError, match='copies'):
        ops.redact_records(tgt.view, {k: v.clone() for k, v in dev.items()}, st)
    # the planes of an NV12 frame from the same buffer
    ty, tc = _yuv_targets(np.random.default_rng(12), 'nv12', 2, H, W, 'pitched')
    st = _style('mosaic', 6)
    ops.redact_records((ty.view, tc[0].view), dev, st, layout='nv12')
    torch.cuda.synchronize()
    skips = [ref.redact_yuv(ty.host[b], *_uv_of('nv12', tc, b), boxes[b] if rotated else boxes[b, :, :4], counts[b], st) for b in range(2)]
    ty.check('records nv12 Y', np.stack([s[0] for s in skips]))
    tc[0].check('records nv12 UV', np.stack([s[1] for s in skips]))


def test_the_launch_pair_is_captured_in_a_graph_and_replays_on_new_frames():
    """No host synchronisation, no allocation, nothing off the stream: the two kernels are captured, and a replay redacts what
    the frames hold then."""
    from mydetection_amd import ops
    H, W = cases.SIZES[0]
    rows = _dev(cases.axis_boxes(H, W)[None])
    st = _style('smooth', 6, pad=1.25)
    frames = torch.zeros((1, H, W, 3), dtype=torch.uint8, device='cuda')
    ops.redact_boxes(frames, rows, st)                               # the workspace exists before the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.redact_boxes(frames, rows, st)
    for seed in (1, 2):
        host = np.random.default_rng(seed).integers(0, 256, size=(1, H, W, 3), dtype=np.uint8)
        frames.copy_(torch.from_numpy(host))
        g.replay()
        torch.cuda.synchronize()
        ref.redact_rgb(host[0], cases.axis_boxes(H, W), None, st)
        assert np.array_equal(frames.cpu().numpy(), host)


def test_bad_arguments_are_refused_with_nothing_launched():
    """MYDET_E_BADARG of the C entry points (include/mydet.h): the frames stay as they were."""
    import ctypes
    from mydetection_amd import _lib, ops
    lib = _lib.lib()
    H, W = 32, 48
    frames = torch.full((1, H, W, 3), 77, dtype=torch.uint8, device='cuda')
    boxes = torch.tensor([[[24.0, 16.0, 20.0, 10.0, 0.0]]], device='cuda')
    cls = torch.zeros((1, 1), dtype=torch.int64, device='cuda')
    ws = torch.empty(lib.mydet_redact_workspace_bytes(1, H, W, 4) // 4, dtype=torch.int32, device='cuda')
    assert ws.numel() == 8 * 12 and lib.mydet_redact_workspace_bytes(1, 33, 49, 16) == 4 * 3 * 4
    for bad in ((0, H, W, 4), (1, 0, W, 4), (1, H, W, 5), (1, H, W, 2), (1, H, W, 66)):
        assert lib.mydet_redact_workspace_bytes(*bad) == -1

    def call(lst=None, workspace=ws, row_bytes=3 * W, **fields):
        lst = ops._list_of_rows(boxes, 0, 1, None, {'cls': cls}) if lst is None else lst
        st = ops.redact_style('smooth', 4).struct()
        for k, v in fields.items():
            setattr(st, k, v)
        return lib.mydet_redact_boxes_rgb_u8(frames.data_ptr(), 1, H, W, 3 * H * W, row_bytes, ctypes.byref(lst), ctypes.byref(st),
                                             None if workspace is None else workspace.data_ptr(), ops._stream())

    for fields in (dict(cell=5), dict(cell=2), dict(cell=66), dict(pad=0.0), dict(pad=-1.0), dict(pad=float('nan')), dict(pad=float('inf')),
                   dict(mode=3), dict(mode=-1), dict(shape=2), dict(n_classes=-1), dict(n_classes=17), dict(workspace=None), dict(row_bytes=3 * W - 1)):
        assert call(**fields) == -1, fields
    no_cls = ops._list_of_rows(boxes, 0, 1, None, {})
    assert call(lst=no_cls, n_classes=1) == -1                       # a filter with a NULL cls plane
    too_many = ops._list_of_rows(boxes, 0, 1, None, {})
    too_many.K = 513
    assert call(lst=too_many) == -1
    torch.cuda.synchronize()
    assert bool((frames == 77).all())
    assert call(mode=_lib.REDACT_SOLID, workspace=None) == 0 and call(lst=no_cls) == 0 and call(n_classes=1) == 0   # class 0 is classes[0]
    torch.cuda.synchronize()
    assert not bool((frames == 77).all())


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
                                          for i in range(n)]))         # packed pixels: a device tensor of them is redacted in place


def _same_objects(a, b):
    assert len(a) == len(b)
    for o, p in zip(a, b):
        assert torch.equal(o.bboxes, p.bboxes) and torch.equal(o.scores, p.scores) and torch.equal(o.cats, p.cats) and o.img_hw == p.img_hw
        assert (o.obj_ids is None) == (p.obj_ids is None) and (o.obj_ids is None or torch.equal(o.obj_ids, p.obj_ids))


def _redacted_from_objects(frames, objs, style):
    """ops.redact_boxes of a list of ImageObjects on a device copy of the frames."""
    from mydetection_amd import ops
    from mydetection_amd.utils.visualization import objects_to_rows
    out = torch.from_numpy(frames).cuda()
    boxes, counts, _, classes, _ = objects_to_rows(objs, out.device)
    return ops.redact_boxes(out, boxes, style, counts=counts, classes=classes)


def test_redact_frames_returns_the_objects_of_predict_frames_and_hides_them(detector):
    from mydetection_amd import ops
    from mydetection_amd.api import Draw, Redact, Tiles, Tracker
    from mydetection_amd.utils.visualization import objects_to_rows
    det = detector
    H, W, B = 150, 200, 2
    kw = dict(input_size=128, conf_thres=0.001)
    frames = _frames(B, H, W, seed=90)
    for n, extra in enumerate(({}, {'tiles': Tiles((96, 128), overlap=0.25)})):
        redact = Redact(MODES[n], shape=('box', 'ellipse')[n], pad=1.25)
        want = det.predict_frames(frames, **kw, **extra)
        assert sum(len(o) for o in want) > 0
        dev_in = torch.from_numpy(frames).cuda()
        objs, redacted = det.redact_frames(dev_in, redact, **kw, **extra)
        _same_objects(objs, want)
        assert redacted.data_ptr() == dev_in.data_ptr()              # a single device tensor is redacted in place
        assert redact.style((H, W)).cell == 4
        expect = _redacted_from_objects(frames, want, redact.style((H, W)))
        assert torch.equal(redacted, expect) and not torch.equal(redacted.cpu(), torch.from_numpy(frames))
        objs2, redacted2 = det.redact_frames(list(frames), redact, **kw, **extra)     # host frames: the batch the call built
        _same_objects(objs2, want)
        assert redacted2.is_cuda and torch.equal(redacted2, expect)
        # annotate_frames(redact=): the redaction first, the overlay on top
        draw = Draw(labels=('class', 'score'), label_height=8)
        objs3, drawn = det.annotate_frames(frames, draw, redact=redact, **kw, **extra)
        _same_objects(objs3, want)
        boxes, counts, scores, classes, ids = objects_to_rows(want, expect.device)
        assert torch.equal(drawn, ops.draw_boxes(expect.clone(), boxes, draw.style((H, W)), counts=counts, scores=scores, classes=classes, ids=ids))
        assert not torch.equal(drawn, expect)
    # tracked, coasting: the returned tracks are what is hidden
    base = _frames(1, H, W, seed=90)[0]
    same = np.stack([base, base])
    trk, trk_ref = Tracker(min_score=0.0005), Tracker(min_score=0.0005)
    redact = Redact('smooth', cell=6)
    for call in range(2):
        want = det.predict_frames(same, tracker=trk_ref, coasting=True, **kw)
        objs, redacted = det.redact_frames(same, redact, tracker=trk, coasting=True, **kw)
        _same_objects(objs, want)
        assert sum(len(o) for o in objs) > 0 and torch.equal(redacted, _redacted_from_objects(same, want, redact.style((H, W))))
    # no detections: the frames come back bit-identical
    objs, redacted = det.redact_frames(frames, Redact('solid', color=(255, 0, 0)), input_size=128, conf_thres=2.0)
    assert all(len(o) == 0 for o in objs) and torch.equal(redacted.cpu(), torch.from_numpy(frames))
    with pytest.raises(ValueError, match='one size'):
        det.redact_frames([frames[0], frames[1, :100]], **kw)
    with pytest.raises(TypeError, match='Redact'):
        det.redact_frames(frames, Draw(), **kw)
    with pytest.raises(TypeError, match='Redact'):
        det.annotate_frames(frames, None, 'mosaic', **kw)


def test_redact_frames_nv12_in_place_and_from_one_surface(detector):
    from mydetection_amd import ops
    from mydetection_amd.api import Redact
    from mydetection_amd.utils.visualization import objects_to_rows
    det = detector
    H, W, B = 150, 200, 2
    kw = dict(input_size=128, conf_thres=0.001)
    frames = _frames(B, H, W, seed=90)
    y = np.ascontiguousarray(frames[:, :, :, 0])
    uv = np.ascontiguousarray(frames[:, ::2, ::2, 1:])
    redact = Redact('mosaic', cell=6)
    want = det.predict_frames_nv12(y, uv, **kw)
    assert sum(len(o) for o in want) > 0
    yd, uvd = torch.from_numpy(y).cuda(), torch.from_numpy(uv).cuda()
    objs, redacted = det.redact_frames_nv12(yd, uvd, redact, **kw)
    _same_objects(objs, want)
    assert redacted[0].data_ptr() == yd.data_ptr() and redacted[1].data_ptr() == uvd.data_ptr()
    ey, euv = torch.from_numpy(y).cuda(), torch.from_numpy(uv).cuda()
    boxes, counts, _, classes, _ = objects_to_rows(want, ey.device)
    ops.redact_boxes_yuv420((ey, euv), 'nv12', boxes, redact.style((H, W)), counts=counts, classes=classes)
    assert torch.equal(yd, ey) and torch.equal(uvd, euv) and not torch.equal(yd.cpu(), torch.from_numpy(y)) and not torch.equal(uvd.cpu(), torch.from_numpy(uv))
    # one surface [B, H*3/2, W]: redacted in place, the same planes
    surface = torch.cat([torch.from_numpy(y), torch.from_numpy(uv).reshape(B, H // 2, W)], dim=1).cuda()
    objs, redacted = det.redact_frames_nv12(surface, None, redact, **kw)
    _same_objects(objs, want)
    assert redacted.data_ptr() == surface.data_ptr() and torch.equal(surface[:, :H], ey) and torch.equal(surface[:, H:].reshape(B, H // 2, W // 2, 2), euv)
    # host planes: the device planes the call built
    objs, redacted = det.redact_frames_yuv((y, uv), 'nv12', redact, **kw)
    assert redacted[0].is_cuda and torch.equal(redacted[0], ey) and torch.equal(redacted[1], euv)
    with pytest.raises(ValueError, match='p010'):
        det.redact_frames_yuv((y.astype(np.uint16), uv.astype(np.uint16)), 'p010', redact, **kw)


def test_redact_launches_what_predict_launches_plus_one(detector):
    """What the docstrings of redact_frames* promise, in the launch counts of an ops.KernelTimer: each call is its predict_frames*
    call plus ONE 'redact_boxes' entry -- RGB and NV12; plain, tiled and tracked --, annotate_frames*(redact=) is that plus ONE
    'draw_boxes', and annotate_frames* without redact= launches what it launched before."""
    from mydetection_amd import ops
    from mydetection_amd.api import Redact, Tiles, Tracker
    det = detector
    kw = dict(input_size=128, conf_thres=0.001)
    frames = _frames(2, 150, 200, seed=90)
    y, uv = np.ascontiguousarray(frames[:, :, :, 0]), np.full((2, 75, 100, 2), 128, np.uint8)

    def launches(method, *args, **extra):
        ops.TIMER = ops.KernelTimer()
        method(*args, **kw, **extra)
        torch.cuda.synchronize()
        return {name: n for name, (n, _, _) in ops.TIMER.summary().items()}

    def plus(counts, *names):
        assert not set(names) & set(counts)
        return dict(counts, **{name: 1 for name in names})

    modes = {'plain': dict, 'tiled': lambda: {'tiles': Tiles((96, 128), overlap=0.25)},
             'tracked': lambda: {'tracker': Tracker(min_score=0.0005)}}     # synthetic weights: keep the low scores alive
    graph, timer = det.use_graph, ops.TIMER
    det.use_graph = False
    try:
        for n, (mode, extra) in enumerate(modes.items()):
            for redact in (Redact(MODES[n]),):
                rgb = launches(det.predict_frames, frames, **extra())
                assert launches(det.redact_frames, frames, redact, **extra()) == plus(rgb, 'redact_boxes'), mode
                assert launches(det.annotate_frames, frames, redact=redact, **extra()) == plus(rgb, 'redact_boxes', 'draw_boxes'), mode
                assert launches(det.annotate_frames, frames, **extra()) == plus(rgb, 'draw_boxes'), mode
                nv12 = launches(det.predict_frames_nv12, y, uv, **extra())
                assert launches(det.redact_frames_nv12, y, uv, redact, **extra()) == plus(nv12, 'redact_boxes'), mode
                assert launches(det.annotate_frames_nv12, y, uv, redact=redact, **extra()) == plus(nv12, 'redact_boxes', 'draw_boxes'), mode
                assert launches(det.annotate_frames_nv12, y, uv, **extra()) == plus(nv12, 'draw_boxes'), mode
    finally:
        det.use_graph, ops.TIMER = graph, timer
