"""GPU tests of the NV12 input path, bit for bit throughout.  The expected RGB frames come from the numpy restatement of the
conversion (_nv12_ref) and go through the EXISTING RGB path (ops.frames_to_input, Detector.predict_frames); nothing is
compared with a tolerance.  ops.nv12_to_rgb against the restatement for all four table rows; ops.nv12_to_input against
frames_to_input in every path of the kernel and every plane layout; the tap-limit fallback; the footprint;
Detector.predict_frames_nv12 / frames_nv12_to_json against predict_frames / frames_to_json."""
import functools
import types

import numpy as np
import pytest
import torch

import _nv12_ref
from _arena import flat_arena

pytestmark = pytest.mark.gpu

FORMATS = ('RGB_1', 'RGB_1_norm')
ROWS = list(_nv12_ref.TABLE)


def _geometry(h, w, name, size=None, div=32):
    from mydetection_amd.api import Detector
    return Detector._geometry(types.SimpleNamespace(divisibe=div), h, w, name, size)


def _taps(n_in, n_out):
    from mydetection_amd.utils.image_ops import resample_tables
    return 0 if n_in == n_out else resample_tables(n_in, n_out)[1].shape[1]


def _pitched(planes, pitch, gap, offset=0):
    """Device copy of [B,R,...] rows of n bytes in ONE allocation of its own with `pitch` bytes between rows, `gap` spare rows
    between frames and `offset` bytes in front; the bytes around the data are 0xA5."""
    a = torch.from_numpy(planes)
    B, R = a.shape[:2]
    n = a[0, 0].numel()
    assert pitch >= n
    buf = torch.full((offset + B * (R + gap) * pitch,), 0xA5, dtype=torch.uint8, device='cuda')
    view = buf[offset:].view(B, R + gap, pitch)[:, :R, :n]
    view.copy_(a.reshape(B, R, n).cuda())
    return view.unflatten(2, a.shape[2:]) if a.dim() == 4 else view


def _layouts(y, uv):
    """name -> (y view, uv view) on the device.  'tight': one frame, packed (dword reads when W % 4 == 0).  'pitched': two frames,
    Y and UV in separate allocations, pitches wider than the picture and multiples of 4, a frame stride larger than the plane
    (dword reads with a partial last quad).  'odd': odd pitches and an odd start address (byte reads)."""
    W, UW = y.shape[2], 2 * uv.shape[2]
    return {
        'tight': (torch.from_numpy(y[:1]).cuda(), torch.from_numpy(uv[:1]).cuda()),
        'pitched': (_pitched(y, (W + 3) // 4 * 4 + 8, 3), _pitched(uv, (UW + 3) // 4 * 4 + 12, 2)),
        'odd': (_pitched(y, (W + 11) | 1, 1, offset=1), _pitched(uv, (UW + 6) | 1, 0, offset=3)),
    }


# (frame h, w), geometry (resize target, (top, left), (Hp, Wp), pad_info): the smallest list that reaches every path
CASES = {
    'pad_only_50x70': ((50, 70), lambda: _geometry(50, 70, 'pad_divisible')),                       # both tables null, two tiles in x
    'y_only_90x40_to_64x40': ((90, 40), lambda: ((64, 40), (0, 8), (64, 64), None)),                # width kept, height resampled
    'down3_120x200_to_40x67': ((120, 200), lambda: ((40, 67), (1, 3), (64, 96), None)),             # 7 taps, several row steps
    'steepest_128x64_to_16x8': ((128, 64), lambda: ((16, 8), (0, 4), (16, 16), None)),              # the tap limit on both axes
    'up_37x53_to_square_64': ((37, 53), lambda: _geometry(37, 53, 'resize_pad_square', 64)),        # odd sizes, upscale: 44 x 64 at (10, 0)
    'up_37x53_odd_origin': ((37, 53), lambda: ((59, 85), (3, 5), (64, 96), None)),                  # odd top / left, a tile seam in x
    'odd_Wp_67': ((90, 71), lambda: ((44, 61), (3, 2), (50, 67), None)),                            # Wp % 4 != 0: one-pixel stores
}


@functools.lru_cache(maxsize=None)
def _case(case, matrix='bt601', full_range=False):
    """(y, uv) numpy planes of two frames and their RGB frames by the numpy restatement -- computed once per case."""
    (h, w), geo = CASES[case]
    y, uv = _nv12_ref.random_nv12(2, h, w, seed=sum(map(ord, case)))
    return y, uv, _nv12_ref.nv12_to_rgb(y, uv, matrix, full_range), geo()


@functools.lru_cache(maxsize=None)
def _want(case, fmt, matrix='bt601', full_range=False):
    """The existing RGB path on the numpy-converted frames."""
    from mydetection_amd import ops
    _, _, rgb, geo = _case(case, matrix, full_range)
    return ops.frames_to_input(torch.from_numpy(rgb).cuda(), geo, fmt)


@pytest.mark.parametrize('matrix,full_range', ROWS)
def test_conversion_of_the_clip_frame(matrix, full_range):
    from mydetection_amd import ops
    y, uv = _nv12_ref.clip_frame()
    want = _nv12_ref.nv12_to_rgb(y, uv, matrix, full_range)
    assert want.shape == (1, 50, 256, 3) and want.min() == 0 and want.max() == 255
    assert all((want[..., c] == 0).any() and (want[..., c] == 255).any() for c in range(3))        # both clip branches, every channel
    got = ops.nv12_to_rgb(torch.from_numpy(y).cuda(), torch.from_numpy(uv).cuda(), matrix, full_range)
    assert got.dtype == torch.uint8 and torch.equal(got.cpu(), torch.from_numpy(want))


@pytest.mark.parametrize('matrix,full_range', ROWS)
def test_conversion_of_an_odd_size_frame(matrix, full_range):
    """37 x 53, Y pitch 64, UV pitch 80, two frames with a frame stride larger than the plane; then the same planes at odd
    addresses into an output view with padded rows (byte reads and byte stores), and one 2-d frame."""
    from mydetection_amd import ops
    y, uv = _nv12_ref.random_nv12(2, 37, 53, seed=12)
    want = torch.from_numpy(_nv12_ref.nv12_to_rgb(y, uv, matrix, full_range))
    yd, uvd = _pitched(y, 64, 5), _pitched(uv, 80, 3)
    assert yd.stride() == (42 * 64, 64, 1) and uvd.stride() == (22 * 80, 80, 2, 1)
    got = ops.nv12_to_rgb(yd, uvd, matrix, full_range)
    assert got.shape == (2, 37, 53, 3) and torch.equal(got.cpu(), want)
    yo, uvo = _layouts(y, uv)['odd']
    assert yo.data_ptr() % 2 == 1 and yo.stride(1) % 2 == 1 and uvo.stride(1) % 2 == 1
    big = torch.full((2, 40, 167), 0x5A, dtype=torch.uint8, device='cuda')
    out = big[:, 1:38, 5:5 + 159].unflatten(2, (53, 3))
    assert ops.nv12_to_rgb(yo, uvo, matrix, full_range, out=out).data_ptr() == out.data_ptr()
    assert torch.equal(out.cpu(), want)
    big[:, 1:38, 5:5 + 159] = 0x5A
    assert bool((big == 0x5A).all()), 'bytes outside the output view were written'
    one = ops.nv12_to_rgb(yd[1], uvd[1], matrix, full_range)
    assert one.shape == (37, 53, 3) and torch.equal(one.cpu(), want[1])


@pytest.mark.parametrize('fmt', FORMATS)
@pytest.mark.parametrize('case', list(CASES))
def test_fused_launch_equals_the_rgb_path(case, fmt):
    from mydetection_amd import _lib, ops
    y, uv, rgb, geo = _case(case)
    (h, w) = CASES[case][0]
    if case == 'pad_only_50x70':
        assert geo[0] is None and geo[2] == (64, 96)
    if case == 'down3_120x200_to_40x67':
        assert _taps(120, 40) == 7 and _taps(200, 67) == 7
    if case == 'steepest_128x64_to_16x8':
        assert _taps(128, 16) == _taps(64, 8) == _lib.FRAMES_MAX_TAPS
    if case == 'up_37x53_to_square_64':
        assert geo[:3] == ((44, 64), (10, 0), (64, 64))
    want = _want(case, fmt)
    assert want.shape == (2, 3) + tuple(geo[2])
    for name, (yd, uvd) in _layouts(y, uv).items():
        got = ops.nv12_to_input(yd, uvd, geo, fmt)
        ref = want[:yd.shape[0]]
        assert got.shape == ref.shape and got.dtype == torch.float32
        assert torch.equal(got, ref), (case, fmt, name, int((got != ref).sum()))
    one = ops.nv12_to_input(torch.from_numpy(y[1]).cuda(), torch.from_numpy(uv[1]).cuda(), geo, fmt)       # [H,W]
    assert torch.equal(one, want[1:])


@pytest.mark.parametrize('fmt', FORMATS)
@pytest.mark.parametrize('matrix,full_range', [r for r in ROWS if r != ('bt601', False)])
def test_fused_launch_with_the_other_table_rows(matrix, full_range, fmt):
    from mydetection_amd import ops
    case = 'down3_120x200_to_40x67'
    y, uv, rgb, geo = _case(case, matrix, full_range)
    assert not np.array_equal(rgb, _case(case)[2])
    yd, uvd = _layouts(y, uv)['pitched']
    assert torch.equal(ops.nv12_to_input(yd, uvd, geo, fmt, matrix, full_range), _want(case, fmt, matrix, full_range))
    assert torch.equal(ops.nv12_to_input(yd, uvd, geo, fmt, matrix=matrix, full_range=full_range), _want(case, fmt, matrix, full_range))


@pytest.mark.parametrize('fmt', FORMATS)
def test_tap_limit_fallback(fmt, monkeypatch):
    """144 x 72 -> 16 x 8 has two taps more than the kernel stages: the planes are converted (ops.yuv420_to_rgb) and take the RGB
    path's own fallback -- the bits frames_to_input gives for the numpy-converted frames."""
    from mydetection_amd import _lib, ops
    assert _taps(144, 16) == _lib.FRAMES_MAX_TAPS + 2
    geo = ((16, 8), (0, 4), (16, 16), None)
    y, uv = _nv12_ref.random_nv12(2, 144, 72, seed=144)
    want = ops.frames_to_input(torch.from_numpy(_nv12_ref.nv12_to_rgb(y, uv)).cuda(), geo, fmt)
    calls = []
    real = ops.yuv420_to_rgb
    monkeypatch.setattr(ops, 'yuv420_to_rgb', lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    yd, uvd = _layouts(y, uv)['pitched']
    got = ops.nv12_to_input(yd, uvd, geo, fmt)
    assert calls == [1] and torch.equal(got, want)
    calls.clear()
    y2, uv2 = _case('steepest_128x64_to_16x8')[:2]                               # at the limit: the fused launch
    ops.nv12_to_input(torch.from_numpy(y2).cuda(), torch.from_numpy(uv2).cuda(), geo, fmt)
    assert calls == []


@pytest.mark.parametrize('case', ['up_37x53_to_square_64', 'down3_120x200_to_40x67', 'odd_Wp_67'])
def test_footprint(case):
    """The output lies between sentinel guard bands: afterwards the bands are untouched and every element of [B,3,Hp,Wp] has
    been written.  (out= takes a contiguous view only, as frames_to_input's: there is no padded-row output to test.)"""
    from mydetection_amd import ops
    y, uv, rgb, geo = _case(case)
    Hp, Wp = geo[2]
    yd, uvd = _layouts(y, uv)['pitched']
    flat, chk = flat_arena(2 * 3 * Hp * Wp, yd.device)
    out = flat.view(2, 3, Hp, Wp)
    assert bool(torch.isnan(out).all())
    got = ops.nv12_to_input(yd, uvd, geo, 'RGB_1_norm', out=out)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr()
    chk.view_defined(case)
    chk.outside_untouched(case)
    assert torch.equal(out, _want(case, 'RGB_1_norm'))


@pytest.fixture(scope='module')
def detector():
    from mydetection_amd import synth
    from mydetection_amd.api import Detector
    from mydetection_amd.models.general import name_to_model
    m, cfg = name_to_model('yolov3_80')
    m.load_state_dict(synth.make_state_dict(m.state_dict(), 'yolov3_80'), strict=True)
    return Detector(model_and_cfg=(m.eval().cuda(), cfg))


def _synthetic_nv12(n, h, w, seed):
    """Planes with structure (synthetic images: luma from their mean, chroma from two channels at half resolution)."""
    from mydetection_amd import synth
    rgb = np.stack([(synth.make_images(1, max(h, w), seed=seed + i)[0, :, :h, :w].permute(1, 2, 0).numpy() * 255).astype(np.uint8)
                    for i in range(n)])
    y = rgb.mean(axis=3).astype(np.uint8)
    uv = np.ascontiguousarray(rgb[:, ::2, ::2, 1:])
    return y, uv


def _same(a, b):
    assert len(a) == len(b)
    for d, e in zip(a, b):
        assert d.img_hw == e.img_hw and d.bboxes.shape == e.bboxes.shape
        assert torch.equal(d.bboxes, e.bboxes) and torch.equal(d.scores, e.scores) and torch.equal(d.cats, e.cats)


def test_predict_frames_nv12_equals_predict_frames(detector):
    det = detector
    kw = dict(input_size=128, conf_thres=0.001)
    y, uv = _synthetic_nv12(3, 90, 120, seed=40)
    rgb = _nv12_ref.nv12_to_rgb(y, uv)
    want = det.predict_frames(rgb, **kw)
    assert sum(len(d) for d in want) > 0 and all(d.img_hw == (90, 120) for d in want)
    _same(det.predict_frames_nv12(torch.from_numpy(y).cuda(), torch.from_numpy(uv).cuda(), **kw), want)    # separate planes, device
    surface = np.concatenate([y, uv.reshape(3, 45, 120)], axis=1)                # a single host surface [B, H*3/2, W]
    assert surface.shape == (3, 135, 120)
    _same(det.predict_frames_nv12(surface, **kw), want)
    _same(det.predict_frames_nv12(torch.from_numpy(surface[1]), **kw), want[1:2])                          # one 2-d surface
    want709 = det.predict_frames(_nv12_ref.nv12_to_rgb(y, uv, 'bt709', True), **kw)
    _same(det.predict_frames_nv12(y, uv, matrix='bt709', full_range=True, **kw), want709)
    rows = det.frames_nv12_to_json(y, uv, [7, 8, 9], **kw)
    assert rows == det.frames_to_json(rgb, [7, 8, 9], **kw) and len(rows) == sum(len(d) for d in want)
    assert det.frames_nv12_to_json(torch.from_numpy(surface).cuda(), None, [7, 8, 9], **kw) == rows
