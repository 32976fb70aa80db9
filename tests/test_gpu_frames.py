"""GPU tests of the video-frame input path: mydet_frames_to_input_f32 (one launch: PIL-exact resize + padding + /255 +
normalisation) against the two-launch path it fuses (resize_bilinear_u8 + preprocess_u8, pinned to Pillow by the golden
preprocessing test) and against Pillow itself, bit for bit; its footprint; and Detector.predict_frames / frames_to_json
against predict_batch / _json_batch on PIL images of the same pixels."""
import types

import numpy as np
import PIL.Image
import pytest
import torch

from _arena import flat_arena

pytestmark = pytest.mark.gpu

FORMATS = ('RGB_1', 'RGB_1_norm')


def _geometry(h, w, name, size=None, div=32):
    from mydetection_amd.api import Detector
    return Detector._geometry(types.SimpleNamespace(divisibe=div), h, w, name, size)


def _frames(b, h, w, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    return torch.from_numpy(rng.integers(0, 256, size=(b, h, w, 3), dtype=np.uint8))


def _two_launch(frames, geo, fmt):
    """The parent path on the same pixels: one resize launch per frame into a zero uint8 batch, then preprocess_u8."""
    from mydetection_amd import ops
    target, (top, left), (Hp, Wp), _ = geo
    B, H, W, _ = frames.shape
    buf = torch.zeros((B, Hp, Wp, 3), dtype=torch.uint8, device=frames.device)
    for n in range(B):
        ops.resize_bilinear_u8(frames[n].contiguous(), target or (H, W), buf[n], top, left)
    return ops.preprocess_u8(buf, (Hp, Wp), fmt)


def _taps(n_in, n_out):
    from mydetection_amd.utils.image_ops import resample_tables
    return 0 if n_in == n_out else resample_tables(n_in, n_out)[1].shape[1]


# (frame h, w), geometry: the smallest shapes at which each mechanism can break
CASES = {
    'square_37x53_to_64': ((37, 53), lambda: _geometry(37, 53, 'resize_pad_square', 64)),          # odd sizes, top/left != 0
    'steep_200x120_to_96': ((200, 120), lambda: _geometry(200, 120, 'resize_pad_divisible', 96)),   # 7 vertical taps, Wp != ow
    'up_48_to_128': ((48, 48), lambda: _geometry(48, 48, 'resize_pad_square', 128)),                # two taps, clamped windows
    'pad_only_50x70': ((50, 70), lambda: _geometry(50, 70, 'pad_divisible')),                       # null tables
    'odd_Wp_67': ((90, 71), lambda: ((44, 61), (3, 2), (50, 67), None)),                            # Wp % 4 != 0: dword stores
    'x_only_40x90_to_40x64': ((40, 90), lambda: ((40, 64), (0, 0), (64, 64), None)),                # horizontal pass alone
    'y_only_90x40_to_64x40': ((90, 40), lambda: ((64, 40), (0, 8), (64, 64), None)),                # vertical pass alone
}


@pytest.mark.parametrize('fmt', FORMATS)
@pytest.mark.parametrize('case', list(CASES))
def test_fused_launch_equals_the_two_launch_path(case, fmt):
    from mydetection_amd import ops
    (h, w), geo = CASES[case]
    geo = geo()
    if case == 'square_37x53_to_64':
        assert geo[1] != (0, 0) and geo[2] == (64, 64)
    if case == 'steep_200x120_to_96':
        assert geo[0] == (96, 58) and geo[2] == (96, 64) and _taps(200, 96) == 7
    for b in (1, 3):
        frames = _frames(b, h, w, seed=100 + b).cuda()
        got = ops.frames_to_input(frames, geo, fmt)
        want = _two_launch(frames, geo, fmt)
        assert got.shape == want.shape == (b, 3) + tuple(geo[2]) and got.dtype == torch.float32
        assert torch.equal(got, want), (case, fmt, b, int((got != want).sum()))


@pytest.mark.parametrize('fmt', FORMATS)
def test_strided_frames_are_read_in_place(fmt):
    """A crop view of a larger device tensor: src_row_bytes > 3 * W and src_img_bytes > H * src_row_bytes."""
    from mydetection_amd import ops
    geo = _geometry(37, 53, 'resize_pad_square', 64)
    for b in (1, 3):
        big = _frames(b, 60, 80, seed=7).cuda()
        crop = big[:, 5:42, 7:60]
        assert crop.shape == (b, 37, 53, 3) and not crop.is_contiguous() and crop.stride(1) == 240 > 3 * 53
        got = ops.frames_to_input(crop, geo, fmt)
        assert torch.equal(got, _two_launch(crop, geo, fmt))
        assert torch.equal(got, ops.frames_to_input(crop.contiguous(), geo, fmt))
    one = ops.frames_to_input(big[1, 5:42, 7:60], geo, fmt)              # [H,W,3]
    assert torch.equal(one[0], got[1])


@pytest.mark.parametrize('fmt', FORMATS)
def test_tap_limit_and_fallback(fmt, monkeypatch):
    """128 rows -> 16 has exactly FRAMES_MAX_TAPS vertical taps (the largest LDS stage); 144 -> 16 has two more and goes
    through the two existing kernels: the same bits either way."""
    from mydetection_amd import _lib, ops
    limit = _lib.FRAMES_MAX_TAPS
    assert _taps(128, 16) == limit and _taps(64, 8) == limit and _taps(144, 16) == limit + 2
    calls = []
    real = ops.resize_bilinear_u8
    monkeypatch.setattr(ops, 'resize_bilinear_u8', lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    for (h, w), fell_back in (((128, 64), False), ((144, 72), True)):
        geo = ((16, 8), (0, 4), (16, 16), None)                         # resize_pad_square to 16
        frames = _frames(2, h, w, seed=h).cuda()
        calls.clear()
        got = ops.frames_to_input(frames, geo, fmt)
        assert bool(calls) == fell_back
        assert torch.equal(got, _two_launch(frames, geo, fmt))
        ref = np.zeros((16, 16, 3), np.uint8)                            # and Pillow itself, at the limit and past it
        ref[geo[1][0]:geo[1][0] + 16, geo[1][1]:geo[1][1] + 8] = np.array(
            PIL.Image.fromarray(frames[1].cpu().numpy()).resize((8, 16), PIL.Image.BILINEAR))
        assert torch.equal(got[1], ops.preprocess_u8(torch.from_numpy(ref).cuda(), (16, 16), fmt)[0])


def test_window_equals_pillow_directly():
    """The steep downscale against image_ops._resize (Pillow) and the host arithmetic of the reference's to_tensor +
    format_tensor_img: the kernel's exactness does not rest on the older kernel alone."""
    from mydetection_amd import ops
    from mydetection_amd.utils import image_ops
    geo = _geometry(200, 120, 'resize_pad_divisible', 96)
    (oh, ow), (Hp, Wp) = geo[0], geo[2]
    frames = _frames(2, 200, 120, seed=11)
    for fmt in FORMATS:
        got = ops.frames_to_input(frames.cuda(), geo, fmt).cpu()
        for b in range(2):
            pil = image_ops._resize(PIL.Image.fromarray(frames[b].numpy()), (oh, ow))
            ref = image_ops.format_tensor_img(image_ops.to_tensor(image_ops._pad(pil, 0, 0, Wp - ow, Hp - oh)), fmt)
            assert torch.equal(got[b, :, :oh, :ow], ref[:, :oh, :ow])
            assert torch.equal(got[b], ref)


@pytest.mark.parametrize('case', ['square_37x53_to_64', 'steep_200x120_to_96', 'odd_Wp_67', 'pad_only_50x70'])
def test_footprint(case):
    """The output lies between sentinel guard bands: afterwards the bands are untouched and every element of
    [B,3,Hp,Wp] has been written (the view starts as NaN sentinels; none remains, nothing is non-finite)."""
    from mydetection_amd import ops
    (h, w), geo = CASES[case]
    geo = geo()
    Hp, Wp = geo[2]
    frames = _frames(3, h, w, seed=5).cuda()
    flat, chk = flat_arena(3 * 3 * Hp * Wp, frames.device)
    out = flat.view(3, 3, Hp, Wp)
    assert bool(torch.isnan(out).all())
    got = ops.frames_to_input(frames, geo, 'RGB_1_norm', out=out)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr()
    chk.view_defined(case)
    chk.outside_untouched(case)
    assert not bool(torch.isnan(out).any())
    assert torch.equal(out, _two_launch(frames, geo, 'RGB_1_norm'))


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


def _same(a, b):
    assert len(a) == len(b)
    for d, e in zip(a, b):
        assert d.img_hw == e.img_hw and d.bboxes.shape == e.bboxes.shape
        assert torch.equal(d.bboxes, e.bboxes) and torch.equal(d.scores, e.scores) and torch.equal(d.cats, e.cats)


def test_predict_frames_equals_predict_batch(detector):
    name, det = detector
    kw = dict(input_size=128, conf_thres=0.001)
    arr = _synthetic_frames(3, 90, 120, seed=40)
    imgs = [PIL.Image.fromarray(a) for a in arr]
    want = det.predict_batch(imgs, **kw)
    assert sum(len(d) for d in want) > 0 and all(d.img_hw == (90, 120) for d in want)
    _same(det.predict_frames(torch.from_numpy(arr).cuda(), **kw), want)             # a device tensor
    assert any(k[0][0] == 3 for k in det._graphs.graphs), 'the second call with this shape is captured'
    _same(det.predict_frames(torch.from_numpy(arr), **kw), want)                    # a host tensor (hipGraph replay)
    _same(det.predict_frames(arr, **kw), want)                                      # a numpy array
    _same(det.predict_frames(arr[1], **kw), det.predict_batch(imgs[1:2], **kw))     # one [H,W,3] frame
    eval_type = 'cxcywhd' if name == 'rapid' else 'x1y1wh'
    rows = det.frames_to_json(arr, [7, 8, 9], eval_type, **kw)
    assert rows == det._json_batch(imgs, [7, 8, 9], eval_type, None, **kw) and len(rows) == sum(len(d) for d in want)


def test_predict_frames_on_a_list_of_two_sizes(detector):
    """resize_pad_divisible gives the two frame sizes two input sizes (two batches); resize_pad_square gives them ONE
    input size, where the frames of both sizes make one batch in input order, as predict_batch builds it."""
    name, det = detector
    a, b = _synthetic_frames(2, 90, 120, seed=50), _synthetic_frames(1, 120, 90, seed=60)
    frames = [a[0], torch.from_numpy(b[0]).cuda(), torch.from_numpy(a[1])]          # numpy, device tensor, host tensor
    imgs = [PIL.Image.fromarray(a[0]), PIL.Image.fromarray(b[0]), PIL.Image.fromarray(a[1])]
    for pre in ('resize_pad_divisible', 'resize_pad_square'):
        kw = dict(input_size=128, conf_thres=0.001, preprocessing=pre)
        want = det.predict_batch(imgs, **kw)
        got = det.predict_frames(frames, **kw)
        assert [d.img_hw for d in got] == [(90, 120), (120, 90), (90, 120)]
        _same(got, want)
        _same(det.predict_frames(frames, **kw), want)
    with pytest.raises(ValueError, match=r'\(90, 120, 4\)'):
        det.predict_frames(np.zeros((90, 120, 4), np.uint8))
