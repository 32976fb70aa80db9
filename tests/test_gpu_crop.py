"""GPU tests of the object chips (mydet_crop_boxes_rgb / mydet_crop_boxes_yuv420) against the numpy restatement of their
sampling rules, tests/_crop_ref.py, on the cases of tests/_crop_cases.py: 96 x 160 and 95 x 157 frames, B = 2 with different
counts, chips 16 x 8 and 32 x 16 (wide stores) and 13 x 7 (element stores), pad 1.0 and 1.25, one, 2 x 2 and 4 x 4 samples per
chip pixel, sources that are contiguous, pitched, and crop views at odd byte offsets inside a larger random buffer.

Axis-aligned boxes and quarter turns are compared bit for bit (every value is settled: tests/test_crop_host.py asserts it for
these same cases).  Rotated boxes must lie inside the restatement's [lo, hi] everywhere, which is equality on every settled
value -- at least 80 % of them, asserted there too."""
import numpy as np
import pytest
import torch

import _crop_cases as cases
import _crop_ref as ref
import _nv12_ref
import _yuv420_ref

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5


def _dev(a, dtype=None):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dtype=dtype).cuda()


def _source(n, kind, seed=0):
    """The case frames of size index n as a device view of the given kind; the backing buffer around it is random and holds
    no pixel of the fill colour."""
    H, W = cases.SIZES[n]
    return cases.Target(np.random.default_rng(50 + seed), 2, H, W, 3, kind, data=cases.frames(H, W), avoid=cases.FILL)


@pytest.mark.parametrize('chip', cases.CHIPS, ids=lambda c: f'{c[0]}x{c[1]}')
@pytest.mark.parametrize('kind', cases.KINDS)
def test_axis_aligned_and_quarter_turn_chips_are_bit_identical(kind, chip):
    from mydetection_amd import ops
    for n, (H, W) in enumerate(cases.SIZES):
        src = _source(n, kind)
        boxes, counts = cases.case_boxes('axis', H, W, chip)
        for pad in cases.PADS:
            want, lo, hi, written = cases.ref_chips('axis', n, chip, pad)
            assert np.array_equal(lo, hi)
            got = ops.crop_boxes(src.view, _dev(boxes), chip, counts=_dev(counts), pad=pad, fill=cases.FILL)
            assert got.dtype == torch.uint8 and tuple(got.shape) == want.shape
            bad = np.argwhere(got.cpu().numpy() != want)
            assert bad.size == 0, (kind, chip, pad, n, len(bad), bad[:5].tolist())
            for fmt in ('RGB_1', 'RGB_1_norm'):
                f = ops.crop_boxes(src.view, _dev(boxes), chip, counts=_dev(counts), pad=pad, fill=cases.FILL, out='input', input_format=fmt)
                expect = ref.to_float(want, fmt == 'RGB_1_norm')
                expect[~written] = 0                                 # new chip buffers are zeroed
                assert f.dtype == torch.float32 and np.array_equal(f.cpu().numpy().view(np.uint32), expect.view(np.uint32)), (kind, chip, pad, fmt)


@pytest.mark.parametrize('chip', cases.CHIPS, ids=lambda c: f'{c[0]}x{c[1]}')
def test_rotated_chips_lie_in_the_interval_of_the_restatement(chip):
    from mydetection_amd import ops
    for n, (H, W) in enumerate(cases.SIZES):
        for kind in ('contiguous', 'odd'):
            src = _source(n, kind)
            boxes, counts = cases.case_boxes('rotated', H, W, chip)
            for pad in cases.PADS:
                value, lo, hi, written = cases.ref_chips('rotated', n, chip, pad)
                got = ops.crop_boxes(src.view, _dev(boxes), chip, counts=_dev(counts), pad=pad, fill=cases.FILL).cpu().numpy()
                inside = (lo <= got) & (got <= hi)
                print(chip, n, kind, pad, 'settled', float((lo == hi)[written].mean()), 'equal to value', float((got == value)[written].mean()))
                assert inside.all(), (chip, n, kind, pad, int((~inside).sum()), np.argwhere(~inside)[:5].tolist())
                # 4-wide rows have no angle: they equal the same boxes at angle 0
                flat = ops.crop_boxes(src.view, _dev(boxes[..., :4]), chip, counts=_dev(counts), pad=pad, fill=cases.FILL)
                zero = boxes.copy()
                zero[..., 4] = 0
                assert torch.equal(flat, ops.crop_boxes(src.view, _dev(zero), chip, counts=_dev(counts), pad=pad, fill=cases.FILL))


@pytest.mark.parametrize('counts', [(5, 2), (0, -1), None], ids=['5-2', '0-bad_class', 'null'])
def test_slots_beyond_the_count_are_not_written(counts):
    from mydetection_amd import ops                                   # -1 is MYDET_COUNT_BAD_CLASS (include/mydet.h)
    M, n = 4, 0
    H, W = cases.SIZES[n]
    src = _source(n, 'contiguous')
    for chip in ((16, 8), (13, 7)):
        rows = cases.axis_rows(H, W, chip)
        picks = np.stack([rows[[1, 16, 3, 18, 0, 2]], rows[[19, 4, 17, 6, 5, 20]]])          # skipped rows among them
        K = picks.shape[1]
        nb = [min(K, M) if counts is None else max(0, min(c, K, M)) for c in (counts or (0, 0))]
        want, _, _, written = ref.chips(src.host, picks, chip, 1.25, cases.FILL, None if counts is None else counts, M)
        assert written.sum(axis=1).tolist() == nb
        for out in ('uint8', 'input'):
            shape = (2, M, 3) + chip if out == 'input' else (2, M) + chip + (3,)
            back = torch.full((2, M + 1) + shape[2:], SENTINEL, dtype=torch.uint8, device='cuda')
            back = back if out == 'uint8' else back.repeat_interleave(4, dim=-1).view(torch.float32)
            dst = back[:, :M]                                        # a frame stride that is not M slots
            before = back.clone()
            got = ops.crop_boxes(src.view, _dev(picks), chip, counts=None if counts is None else _dev(np.array(counts, np.int32)), max_per_frame=M,
                                 pad=1.25, fill=cases.FILL, out=out, input_format='RGB_1_norm', dst=dst)
            assert got is dst
            expect = want if out == 'uint8' else ref.to_float(want, True)
            g = got.cpu().numpy()
            for b in range(2):
                for m in range(M):
                    if written[b, m]:
                        assert np.array_equal(g[b, m], expect[b, m]), (counts, chip, out, b, m)
                    else:                                            # the sentinel, byte for byte
                        assert torch.equal(got[b, m].contiguous().view(torch.uint8), before[b, m].contiguous().view(torch.uint8)), (counts, chip, out, b, m)
            assert torch.equal(back[:, M].contiguous().view(torch.uint8), before[:, M].contiguous().view(torch.uint8))
            skipped = [(b, m) for b in range(2) for m in range(M) if written[b, m] and not ref.valid_row(picks[b, m])]
            assert counts == (0, -1) or skipped
            for b, m in skipped:
                assert (want[b, m] == np.asarray(cases.FILL, np.uint8)).all()


def test_nothing_outside_the_view_is_read():
    """Odd-offset views inside a random backing buffer that has no pixel of the fill colour: chips of boxes hanging over each
    edge equal the restatement, which sees the view alone -- a tap that read the backing buffer would show."""
    from mydetection_amd import ops
    for n, (H, W) in enumerate(cases.SIZES):
        src = _source(n, 'odd', seed=n)
        assert not (src.back == np.asarray(cases.FILL, np.uint8)).all(axis=-1)[:, :2].any()
        chip = (16, 8)
        a, b, c = cases.SCALES
        rows = np.array([[0.0, H / 2, 8 * b, 16 * b, 0], [W + 0.0, H / 2, 8 * b, 16 * b, 0], [W / 2, 0.0, 8 * b, 16 * a, 0],
                         [W / 2, H + 0.0, 8 * a, 16 * b, 0], [0.5, 0.5, 8 * c, 16 * c, 0], [W - 0.5, H - 0.5, 8 * c, 16 * c, 180],
                         [-0.5, 10.0, 8 * a, 16 * a, 90], [W + 0.5, H + 0.5, 8 * a, 16 * a, 0], [W / 2, H / 2, 8 * 40, 16 * 10, 0]], dtype=np.float32)
        boxes = np.stack([rows, rows[::-1]])
        want, lo, hi, _ = ref.chips(src.host, boxes, chip, 1.0, cases.FILL)
        assert np.array_equal(lo, hi)
        fills = (want == np.asarray(cases.FILL, np.uint8)).all(axis=-1)
        assert 0.2 < fills[:, :8].mean() < 0.8                        # the boxes really hang over the edges
        got = ops.crop_boxes(src.view, _dev(boxes), chip, fill=cases.FILL).cpu().numpy()
        assert np.array_equal(got, want), np.argwhere(got != want)[:5].tolist()


@pytest.mark.parametrize('layout', _yuv420_ref.LAYOUTS)
def test_every_420_layout_gives_the_chips_of_its_rgb_frames(layout):
    from mydetection_amd import ops
    H, W = cases.SIZES[1]                                             # odd H and W
    chip = (16, 8)
    boxes = np.concatenate([cases.case_boxes('axis', H, W, chip)[0][:, :16], cases.case_boxes('rotated', H, W, chip)[0]], axis=1)
    counts = _dev(np.array([boxes.shape[1], 11], np.int32))
    host = _yuv420_ref.random_planes(layout, 2, H, W, seed=31)
    planes = tuple(torch.from_numpy(p.view(np.int16) if p.dtype == np.uint16 else p).cuda() for p in host)
    for matrix, full in (('bt601', False), ('bt709', True), ('bt601', True), ('bt709', False)):
        rgb = ops.yuv420_to_rgb(planes, layout, matrix, full)
        for out, fmt, chip_size in (('uint8', None, chip), ('input', 'RGB_1_norm', chip), ('uint8', None, (13, 7))):
            kw = dict(counts=counts, pad=1.25, fill=cases.FILL, out=out, input_format=fmt)
            want = ops.crop_boxes(rgb, _dev(boxes), chip_size, **kw)
            got = ops.crop_boxes_yuv420(planes, layout, _dev(boxes), chip_size, matrix=matrix, full_range=full, **kw)
            assert torch.equal(got.view(torch.uint8), want.view(torch.uint8)), (layout, matrix, full, out)
            assert int((want.view(torch.uint8) != 0).sum()) > 1000
        if layout == 'nv12':                                          # and against the restatement, on the restated conversion
            frames = _nv12_ref.nv12_to_rgb(host[0], host[1], matrix, full)
            assert np.array_equal(frames, rgb.cpu().numpy())
            axis = boxes[:, :16]
            want, lo, hi, _ = ref.chips(frames, axis, chip, 1.25, cases.FILL)
            assert np.array_equal(lo, hi)
            got = ops.crop_boxes_yuv420(planes, layout, _dev(axis), chip, pad=1.25, fill=cases.FILL, matrix=matrix, full_range=full)
            assert np.array_equal(got.cpu().numpy(), want)
    # pitched planes (aligned wide reads with a partial last group) and odd-offset planes (sample by sample) give the same chips
    if layout in ('nv12', 'i420', 'p010'):
        base = ops.crop_boxes_yuv420(planes, layout, _dev(boxes), chip, counts=counts, fill=cases.FILL)
        for off in (0, 1):
            views = []
            for p in planes:
                shape = list(p.shape)
                shape[1] += 3
                shape[2] += 4 + off
                big = torch.randint(0, 256, shape, device='cuda').to(p.dtype)
                v = big[:, off:off + p.shape[1], off:off + p.shape[2]]
                v.copy_(p)
                views.append(v)
            assert torch.equal(ops.crop_boxes_yuv420(tuple(views), layout, _dev(boxes), chip, counts=counts, fill=cases.FILL), base), (layout, off)


def _records(rng, B, H, W, counts, rotated):
    """A full record buffer (numpy int32 [B, words]) of boxes at multiples of 1/8, and its boxes [B, 512, 5]."""
    from mydetection_amd import _lib
    words = _lib.REC_ROT_WORDS if rotated else _lib.REC_WORDS
    rec = np.zeros((B, words), dtype=np.int32)
    boxes = np.zeros((B, 512, 5), dtype=np.float32)
    eighths = lambda lo, hi: rng.integers(int(lo * 8), int(hi * 8) + 1, size=(B, 512)).astype(np.float64) / 8.0
    boxes[..., 0], boxes[..., 1] = eighths(0, W), eighths(0, H)
    boxes[..., 2], boxes[..., 3] = eighths(2, 40), eighths(2, 40)
    if rotated:
        boxes[..., 4] = rng.uniform(-180, 180, size=(B, 512))
    rec[:, _lib.REC_COUNT] = counts
    rec[:, _lib.REC_BBOX:_lib.REC_SCORE] = boxes[..., :4].reshape(B, -1).view(np.int32)
    rec[:, _lib.REC_SCORE:_lib.REC_CLASS] = rng.uniform(0, 1, size=(B, 512)).astype(np.float32).view(np.int32)
    if rotated:
        rec[:, _lib.REC_ANGLE:] = boxes[..., 4].view(np.int32)
    return rec, boxes


@pytest.mark.parametrize('rotated', [False, True])
def test_crop_records_reads_a_full_record_buffer_in_place(rotated):
    from mydetection_amd import ops
    n = 1
    H, W = cases.SIZES[n]
    counts = np.array([512, 37], np.int32)
    rec, boxes = _records(np.random.default_rng(7 + rotated), 2, H, W, counts, rotated)
    dev = ops.record_views(torch.from_numpy(rec).cuda())
    src = _source(n, 'pitched')
    dense = _dev(boxes if rotated else boxes[..., :4])
    for kw in (dict(out='uint8'), dict(out='input', input_format='RGB_1', max_per_frame=40, pad=1.25)):
        got = ops.crop_records(src.view, dev, (16, 8), fill=cases.FILL, **kw)
        want = ops.crop_boxes(src.view, dense, (16, 8), counts=_dev(counts), fill=cases.FILL, **kw)
        assert got.shape[1] == kw.get('max_per_frame', 512) and torch.equal(got.view(torch.uint8), want.view(torch.uint8))
        assert int((got[1, 37:].view(torch.uint8) != 0).sum()) == 0 and int((got[1, :37].view(torch.uint8) != 0).sum()) > 0
    # from NV12 planes too
    y, uv = (torch.from_numpy(p).cuda() for p in _nv12_ref.random_nv12(2, H, W, seed=4))
    got = ops.crop_records((y, uv), dev, (13, 7), layout='nv12', max_per_frame=64, matrix='bt709')
    want = ops.crop_boxes_yuv420((y, uv), 'nv12', dense, (13, 7), counts=_dev(counts), max_per_frame=64, matrix='bt709')
    assert torch.equal(got, want)
    assert torch.equal(dev['records'].cpu(), torch.from_numpy(rec))   # read only
    with pytest.raises(ValueError, match='copies'):
        ops.crop_records(src.view, {k: v.clone() for k, v in dev.items()}, (16, 8))


def test_unaligned_destinations_take_the_element_stores_with_the_same_result():
    from mydetection_amd import ops
    n = 0
    H, W = cases.SIZES[n]
    src = _source(n, 'contiguous')
    chip = (16, 8)
    boxes, counts = cases.case_boxes('axis', H, W, chip)
    K = boxes.shape[1]
    for out, dtype in (('uint8', torch.uint8), ('input', torch.float32)):
        want = ops.crop_boxes(src.view, _dev(boxes), chip, counts=_dev(counts), fill=cases.FILL, out=out)
        per = 3 * 16 * 8
        flat = torch.zeros(2 * K * (per + 1) + 1, dtype=dtype, device='cuda')
        dst = flat[1:].view(2, K, per + 1)[:, :, :per].view((2, K) + tuple(want.shape[2:]))      # odd base, odd slot stride
        assert dst.data_ptr() % (4 * dst.element_size()) != 0
        got = ops.crop_boxes(src.view, _dev(boxes), chip, counts=_dev(counts), fill=cases.FILL, out=out, dst=dst)
        assert got is dst and torch.equal(got, want)


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
                                          for i in range(n)]))


def _same_objects(a, b):
    assert len(a) == len(b)
    for o, p in zip(a, b):
        assert torch.equal(o.bboxes, p.bboxes) and torch.equal(o.scores, p.scores) and torch.equal(o.cats, p.cats) and o.img_hw == p.img_hw
        assert (o.obj_ids is None) == (p.obj_ids is None) and (o.obj_ids is None or torch.equal(o.obj_ids, p.obj_ids))


def _check_chips(det, source, layout, objs, got, chips, **yuv):
    """chips[b][k] equals the dense call on row k of objs[b].bboxes."""
    from mydetection_amd import ops
    assert len(got) == len(objs)
    kw = chips.kwargs(det.model.input_format)
    kw.pop('max_per_frame')
    total = 0
    for b, (o, c) in enumerate(zip(objs, got)):
        n = min(len(o), chips.max_per_frame)
        assert c.shape[0] == n and c.is_cuda
        if n == 0:
            continue
        rows = o.bboxes.to('cuda', torch.float32)[None, :n]
        assert rows.shape[2] == 5                                     # the rotated model: cxcywhd rows
        if layout is None:
            want = ops.crop_boxes(source[b:b + 1], rows, **kw)
        else:
            want = ops.crop_boxes_yuv420(tuple(p[b:b + 1] for p in source), layout, rows, **kw, **yuv)
        assert torch.equal(c, want[0]), (b, n)
        total += n
    views = [c for c in got if c.shape[0]]
    assert all(v.untyped_storage().data_ptr() == views[0].untyped_storage().data_ptr() for v in views)      # ONE buffer
    return total


def test_crop_frames_returns_the_objects_of_predict_frames_and_their_upright_chips(detector):
    from mydetection_amd.api import Chips, Tiles, Tracker
    det = detector
    H, W, B = 150, 200, 2
    kw = dict(input_size=128, conf_thres=0.001)
    frames = _frames(B, H, W, seed=90)
    dev = torch.from_numpy(frames).cuda()
    for extra in ({}, {'tiles': Tiles((96, 128), overlap=0.25)}):
        for chips in (Chips(size=(32, 16), pad=1.2, max_per_frame=8), Chips(size=(13, 7), out='uint8', fill=(9, 8, 7), max_per_frame=64)):
            want = det.predict_frames(frames, **kw, **extra)
            assert sum(len(o) for o in want) > 0
            objs, got = det.crop_frames(dev, chips, **kw, **extra)
            _same_objects(objs, want)
            assert _check_chips(det, dev, None, objs, got, chips) > 0
            assert got[0].dtype == (torch.uint8 if chips.out == 'uint8' else torch.float32)
            objs2, got2 = det.crop_frames(list(frames), chips, **kw, **extra)      # host frames
            _same_objects(objs2, want)
            assert all(torch.equal(a, b) for a, b in zip(got, got2))
    assert max(len(o) for o in want) > 8                             # the cap of max_per_frame was met above
    # a tracker: the chips show the tracks' filtered boxes
    trk, trk_ref = Tracker(min_score=0.0005), Tracker(min_score=0.0005)
    chips = Chips(size=(16, 8), max_per_frame=32)
    both = np.stack([frames[0], frames[0]])
    for call in range(2):
        want = det.predict_frames(both, tracker=trk_ref, **kw)
        objs, got = det.crop_frames(both, chips, tracker=trk, **kw)
        _same_objects(objs, want)
        assert _check_chips(det, torch.from_numpy(both).cuda(), None, objs, got, chips) > 0
    # no detections: empty views
    objs, got = det.crop_frames(frames, input_size=128, conf_thres=2.0)
    assert all(len(o) == 0 for o in objs) and [tuple(c.shape) for c in got] == [(0, 3, 128, 64)] * B


def test_crop_frames_nv12_cuts_the_chips_out_of_the_planes(detector):
    from mydetection_amd.api import Chips
    det = detector
    H, W, B = 150, 200, 2
    kw = dict(input_size=128, conf_thres=0.001)
    frames = _frames(B, H, W, seed=90)
    y = np.ascontiguousarray(frames[:, :, :, 0])
    uv = np.ascontiguousarray(frames[:, ::2, ::2, 1:])
    chips = Chips(size=(32, 16), pad=1.2, max_per_frame=16)
    want = det.predict_frames_nv12(y, uv, matrix='bt709', **kw)
    assert sum(len(o) for o in want) > 0
    yd, uvd = torch.from_numpy(y).cuda(), torch.from_numpy(uv).cuda()
    objs, got = det.crop_frames_nv12(yd, uvd, chips, matrix='bt709', **kw)
    _same_objects(objs, want)
    assert _check_chips(det, (yd, uvd), 'nv12', objs, got, chips, matrix='bt709') > 0
    # the 10-bit layouts are accepted: crops only read
    y10, uv10 = (y.astype(np.uint16) << 8), (uv.astype(np.uint16) << 8)
    want10 = det.predict_frames_yuv((y10, uv10), 'p010', matrix='bt709', **kw)
    objs10, got10 = det.crop_frames_yuv((y10, uv10), 'p010', chips, matrix='bt709', **kw)
    _same_objects(objs10, want10)
    _same_objects(objs10, want)                                       # v10 = 4 * s reduces to s
    assert all(torch.equal(a, b) for a, b in zip(got, got10))
