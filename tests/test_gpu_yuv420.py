"""GPU tests of the 4:2:0 input path (nv12, nv21, i420, yv12, p010, i010), bit for bit throughout.  The expected RGB frames come
from the numpy helper (_yuv420_ref repacks any layout to NV12 planes, _nv12_ref converts those) and go through the EXISTING RGB
path (ops.frames_to_input, Detector.predict_frames); nothing is compared with a tolerance.  Every layout of a case stores the
same 8-bit samples (the 16-bit ones as 10-bit values that reduce to them, with random ignored bits), so one reference per
case serves all layouts.  Geometries, shapes and the detector fixture are those of the NV12 tests."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import _nv12_ref
import _yuv420_ref as ref
from _arena import flat_arena
from test_gpu_nv12 import CASES, FORMATS, ROWS, _same, _synthetic_nv12, _taps, detector  # noqa: F401

pytestmark = pytest.mark.gpu

LAYOUTS = ref.LAYOUTS
# bytes a plane's address, pitch and frame stride must be multiples of for the kernels' wide reads (include/mydet.h)
WIDE_RULE = {'nv12': (4, 4), 'nv21': (4, 4), 'i420': (4, 2, 2), 'yv12': (4, 2, 2), 'p010': (8, 8), 'i010': (8, 4, 4)}


def _dev(a):
    """A numpy plane on the device; 16-bit words as int16 (the same bits)."""
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).cuda()


def _place(a, pitch, gap, offset=0):
    """Device copy of the numpy plane [B,R,...] in ONE allocation of its own with `pitch` bytes between rows, `gap` spare rows
    between frames and `offset` bytes in front; the bytes around the data are 0xA5."""
    es = a.dtype.itemsize
    B, R = a.shape[:2]
    n = int(np.prod(a.shape[2:]))
    assert pitch >= n * es and pitch % es == 0 and offset % es == 0
    buf = torch.full((offset + B * (R + gap) * pitch,), 0xA5, dtype=torch.uint8, device='cuda')
    flat = buf[offset:].view(torch.int16) if es == 2 else buf[offset:]
    view = flat.view(B, R + gap, pitch // es)[:, :R, :n]
    view.copy_(_dev(a).reshape(B, R, n))
    return view.unflatten(2, a.shape[2:]) if a.ndim == 4 else view


def _wide(planes, layout):
    """The device planes lie on the wide-read side of the rule."""
    return all((t.data_ptr() | t.stride(0) * t.element_size() | t.stride(1) * t.element_size()) % m == 0
               for t, m in zip(planes, WIDE_RULE[layout]))


def _row_bytes(a):
    return int(np.prod(a.shape[2:])) * a.dtype.itemsize


def _pitched(planes):
    """Two frames, every plane in an allocation of its own, pitches wider than the picture and frame strides larger than the
    plane, all multiples of 8: wide reads, with a partial last quad when W % 4 != 0."""
    return tuple(_place(a, (_row_bytes(a) + 7) // 8 * 8 + 8 * (i + 1), 3 - i) for i, a in enumerate(planes))


def _below(planes):
    """The far side of the wide-read rule: odd addresses and pitches for 8-bit samples; even ones that are no multiples of 4 for
    16-bit words."""
    if planes[0].dtype == np.uint8:
        return tuple(_place(a, (_row_bytes(a) + 6 + 5 * i) | 1, 1, offset=1 + 2 * i) for i, a in enumerate(planes))
    return tuple(_place(a, (_row_bytes(a) + 3) // 4 * 4 + 6 + 4 * i, 1, offset=2 + 4 * i) for i, a in enumerate(planes))


def _layouts(planes, layout):
    """name -> device planes: 'tight' (one frame, packed), 'pitched' (wide reads), 'below' (reads by samples)."""
    out = {'tight': tuple(_dev(a[:1]) for a in planes), 'pitched': _pitched(planes), 'below': _below(planes)}
    assert _wide(out['pitched'], layout) and not _wide(out['below'], layout)
    for t in out['below']:
        es, bits = t.element_size(), t.data_ptr() | t.stride(1) * t.element_size()
        assert bits % 2 == 1 if es == 1 else (bits % 2 == 0 and bits % 4 == 2)
    return out


@functools.lru_cache(maxsize=None)
def _case(case, matrix='bt601', full_range=False):
    """NV12 planes of two frames, their RGB frames by the numpy restatement and the geometry -- computed once per case."""
    (h, w), geo = CASES[case]
    y, uv = _nv12_ref.random_nv12(2, h, w, seed=sum(map(ord, case)) + 1)
    return y, uv, _nv12_ref.nv12_to_rgb(y, uv, matrix, full_range), geo()


@functools.lru_cache(maxsize=None)
def _planes(case, layout):
    """The same samples stored in `layout` (numpy, storage order); _yuv420_ref asserts that they repack to the NV12 planes."""
    y, uv = _case(case)[:2]
    return ref.from_nv12(y, uv, layout, seed=len(case))


@functools.lru_cache(maxsize=None)
def _want(case, fmt, matrix='bt601', full_range=False):
    """The existing RGB path on the numpy-converted frames."""
    from mydetection_amd import ops
    _, _, rgb, geo = _case(case, matrix, full_range)
    return ops.frames_to_input(torch.from_numpy(rgb).cuda(), geo, fmt)


@pytest.mark.parametrize('matrix,full_range', ROWS)
@pytest.mark.parametrize('layout', LAYOUTS)
def test_conversion_of_the_clip_frame(layout, matrix, full_range):
    from mydetection_amd import ops
    planes = ref.clip_frame(layout)
    want = ref.to_rgb(planes, layout, matrix, full_range)
    assert want.shape == (1, 50, 256, 3) and np.array_equal(want, _nv12_ref.nv12_to_rgb(*_nv12_ref.clip_frame(), matrix, full_range))
    assert all((want[..., c] == 0).any() and (want[..., c] == 255).any() for c in range(3))        # both clip branches, every channel
    if layout in ref.WORDS:
        v10 = planes[0] >> 6 if layout == 'p010' else planes[0] & 1023
        assert {1021, 1022, 1023} <= set(np.unique(v10).tolist())
        assert all(((p & 63) if layout == 'p010' else (p >> 10)).any() for p in planes)            # non-zero ignored bits
    got = ops.yuv420_to_rgb(tuple(_dev(p) for p in planes), layout, matrix, full_range)
    assert got.dtype == torch.uint8 and torch.equal(got.cpu(), torch.from_numpy(want))


@pytest.mark.parametrize('matrix,full_range', ROWS)
@pytest.mark.parametrize('layout', LAYOUTS)
def test_conversion_of_an_odd_size_frame(layout, matrix, full_range):
    """37 x 53, random samples and (16-bit) random ignored bits: two frames with pitches wider than the picture and a frame
    stride larger than the plane; the same planes on the far side of the wide-read rule into an output view with padded rows;
    one 2-d frame."""
    from mydetection_amd import ops
    planes = ref.random_planes(layout, 2, 37, 53, seed=12)
    want = torch.from_numpy(ref.to_rgb(planes, layout, matrix, full_range))
    pd = _pitched(planes)
    assert _wide(pd, layout) and all(t.stride(1) * t.element_size() > _row_bytes(a) and t.stride(0) > t.shape[1] * t.stride(1)
                                     for t, a in zip(pd, planes))
    got = ops.yuv420_to_rgb(pd, layout, matrix, full_range)
    assert got.shape == (2, 37, 53, 3) and torch.equal(got.cpu(), want)
    pb = _layouts(planes, layout)['below']
    big = torch.full((2, 40, 167), 0x5A, dtype=torch.uint8, device='cuda')
    out = big[:, 1:38, 5:5 + 159].unflatten(2, (53, 3))
    assert ops.yuv420_to_rgb(pb, layout, matrix, full_range, out=out).data_ptr() == out.data_ptr()
    assert torch.equal(out.cpu(), want)
    big[:, 1:38, 5:5 + 159] = 0x5A
    assert bool((big == 0x5A).all()), 'bytes outside the output view were written'
    one = ops.yuv420_to_rgb(tuple(t[1] for t in pd), layout, matrix, full_range)
    assert one.shape == (37, 53, 3) and torch.equal(one.cpu(), want[1])


@pytest.mark.parametrize('fmt', FORMATS)
@pytest.mark.parametrize('case', list(CASES))
@pytest.mark.parametrize('layout', LAYOUTS)
def test_fused_launch_equals_the_rgb_path(layout, case, fmt):
    from mydetection_amd import _lib, ops
    geo = _case(case)[3]
    if case == 'down3_120x200_to_40x67':
        assert _taps(120, 40) == 7 and _taps(200, 67) == 7
    if case == 'steepest_128x64_to_16x8':
        assert _taps(128, 16) == _taps(64, 8) == _lib.FRAMES_MAX_TAPS
    planes = _planes(case, layout)
    want = _want(case, fmt)
    assert want.shape == (2, 3) + tuple(geo[2])
    for name, pd in _layouts(planes, layout).items():
        got = ops.yuv420_to_input(pd, layout, geo, fmt)
        wanted = want[:pd[0].shape[0]]
        assert got.shape == wanted.shape and got.dtype == torch.float32
        assert torch.equal(got, wanted), (layout, case, fmt, name, int((got != wanted).sum()))
    one = ops.yuv420_to_input(tuple(_dev(a[1]) for a in planes), layout, geo, fmt)                   # 2-d planes
    assert torch.equal(one, want[1:])


@pytest.mark.parametrize('fmt', FORMATS)
@pytest.mark.parametrize('matrix,full_range', [r for r in ROWS if r != ('bt601', False)])
@pytest.mark.parametrize('layout', ['i420', 'p010'])
def test_fused_launch_with_the_other_table_rows(layout, matrix, full_range, fmt):
    from mydetection_amd import ops
    case = 'down3_120x200_to_40x67'
    rgb, geo = _case(case, matrix, full_range)[2:]
    assert not np.array_equal(rgb, _case(case)[2])
    pd = _pitched(_planes(case, layout))
    assert torch.equal(ops.yuv420_to_input(pd, layout, geo, fmt, matrix, full_range), _want(case, fmt, matrix, full_range))
    assert torch.equal(ops.yuv420_to_input(pd, layout, geo, fmt, matrix=matrix, full_range=full_range), _want(case, fmt, matrix, full_range))


def test_torch_uint16_planes_are_the_same_bits():
    from mydetection_amd import ops
    if not hasattr(torch, 'uint16'):
        assert ops.yuv420_sample_dtypes(2) == (torch.int16,)
        return
    planes = ref.random_planes('p010', 1, 37, 53, seed=5)
    pd = tuple(_dev(a) for a in planes)
    assert torch.equal(ops.yuv420_to_rgb(tuple(t.view(torch.uint16) for t in pd), 'p010'), ops.yuv420_to_rgb(pd, 'p010'))


@pytest.mark.parametrize('case', ['up_37x53_odd_origin', 'down3_120x200_to_40x67'])
def test_nv12_through_the_new_entry_points_equals_the_nv12_ops(case):
    """The two mydet_nv12_* C entry points, which no Python op calls, through ctypes on the tensors' pointers and byte strides:
    the bits ops.yuv420_to_rgb / ops.yuv420_to_input give for layout 'nv12' (and those the restatement gives)."""
    from mydetection_amd import _lib, ops
    lib = _lib.lib()
    y, uv, rgb, geo = _case(case)
    for name, (yd, uvd) in _layouts((y, uv), 'nv12').items():
        B, H, W = yd.shape
        src = (yd.data_ptr(), yd.stride(0), yd.stride(1), uvd.data_ptr(), uvd.stride(0), uvd.stride(1), B, H, W)
        for matrix, full_range in (('bt601', False), ('bt709', True)):
            got = torch.full((B, H, W, 3), 0x5A, dtype=torch.uint8, device='cuda')
            code = lib.mydet_nv12_to_rgb_u8(*src, got.data_ptr(), got.stride(0), got.stride(1), ops.yuv_matrix_id(matrix), int(full_range),
                                            ops._stream())
            assert code == 0 and torch.equal(got, ops.yuv420_to_rgb((yd, uvd), 'nv12', matrix, full_range)), (name, matrix)
        assert torch.equal(got.cpu(), torch.from_numpy(_case(case, 'bt709', True)[2][:B])), name
        assert torch.equal(ops.nv12_to_rgb(yd, uvd).cpu(), torch.from_numpy(rgb[:B])), name
        for fmt in FORMATS:
            out, _, _, taps, tail = ops._input_window('nv12', B, H, W, yd.device, geo, fmt, None)
            assert taps <= _lib.FRAMES_MAX_TAPS
            out.fill_(float('nan'))
            code = lib.mydet_nv12_to_input_f32(*src, 0, 0, *tail, ops._stream())
            assert code == 0 and torch.equal(out, ops.yuv420_to_input((yd, uvd), 'nv12', geo, fmt)), (name, fmt)


@pytest.mark.parametrize('layout', ['nv21', 'yv12', 'i010'])
def test_tap_limit_fallback(layout, monkeypatch):
    """144 x 72 -> 16 x 8 has two taps more than the kernel stages: the planes are converted (ops.yuv420_to_rgb, exactly once)
    and take the RGB path's own fallback -- the bits frames_to_input gives for the numpy-converted frames."""
    from mydetection_amd import _lib, ops
    assert _taps(144, 16) == _lib.FRAMES_MAX_TAPS + 2
    geo = ((16, 8), (0, 4), (16, 16), None)
    y, uv = _nv12_ref.random_nv12(2, 144, 72, seed=144)
    want = ops.frames_to_input(torch.from_numpy(_nv12_ref.nv12_to_rgb(y, uv)).cuda(), geo, 'RGB_1_norm')
    calls = []
    real = ops.yuv420_to_rgb
    monkeypatch.setattr(ops, 'yuv420_to_rgb', lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    got = ops.yuv420_to_input(_pitched(ref.from_nv12(y, uv, layout, seed=7)), layout, geo, 'RGB_1_norm')
    assert calls == [1] and torch.equal(got, want)
    calls.clear()
    case = 'steepest_128x64_to_16x8'                                             # at the limit: the fused launch
    got = ops.yuv420_to_input(tuple(_dev(a) for a in _planes(case, layout)), layout, geo, 'RGB_1_norm')
    assert calls == [] and torch.equal(got, _want(case, 'RGB_1_norm'))


@pytest.mark.parametrize('case', ['up_37x53_to_square_64', 'down3_120x200_to_40x67', 'odd_Wp_67'])
@pytest.mark.parametrize('layout', ['yv12', 'p010'])
def test_footprint(layout, case):
    """The output lies between sentinel guard bands: afterwards the bands are untouched and every element of [B,3,Hp,Wp] has
    been written."""
    from mydetection_amd import ops
    geo = _case(case)[3]
    Hp, Wp = geo[2]
    pd = _pitched(_planes(case, layout))
    flat, chk = flat_arena(2 * 3 * Hp * Wp, pd[0].device)
    out = flat.view(2, 3, Hp, Wp)
    assert bool(torch.isnan(out).all())
    got = ops.yuv420_to_input(pd, layout, geo, 'RGB_1_norm', out=out)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr()
    chk.view_defined(case)
    chk.outside_untouched(case)
    assert torch.equal(out, _want(case, 'RGB_1_norm'))


def test_argument_codes_of_the_c_entries():
    """Every refused call returns MYDET_E_BADARG and leaves a sentinel-filled output as it was: nothing was launched."""
    from mydetection_amd import _lib
    lib = _lib.lib()
    H, W, bad = 8, 9, -1
    u8 = torch.full((4096,), 77, dtype=torch.uint8, device='cuda')
    p = u8.data_ptr()
    assert p % 16 == 0
    rgb_out = torch.full((H, W, 3), 0x5A, dtype=torch.uint8, device='cuda')
    f32_out = torch.full((3, H, W), -7.0, device='cuda')
    sizes = dict(B=1, H=H, W=W)

    def src_of(layout=0, planes=(p, p + 1024, None), img=(0, 0, 0), row=(32, 32, 32), matrix=0, full=0):
        return _lib.Yuv420Src((ctypes.c_void_p * 3)(*planes), (ctypes.c_int64 * 3)(*img), (ctypes.c_int64 * 3)(*row), layout, matrix, full, 0)

    def rgb(null=False, dst=True, dr=3 * W, di=0, B=1, H=H, W=W, **k):
        src = src_of(**k)
        return lib.mydet_yuv420_to_rgb_u8(None if null else ctypes.byref(src), B, H, W, rgb_out.data_ptr() if dst else None, di, dr, None)

    def fused(null=False, out=True, B=1, H=H, W=W, Hp=H, Wp=W, **k):                # no resize: null tables
        src = src_of(**k)
        return lib.mydet_yuv420_to_input_f32(None if null else ctypes.byref(src), B, H, W, f32_out.data_ptr() if out else None, Hp, Wp,
                                             H, W, 0, 0, None, None, 0, None, None, 0, 0, None, None, None)
    three = (p, p + 1024, p + 2048)
    refused = [
        dict(null=True), dict(layout=5), dict(layout=-1), dict(matrix=2), dict(matrix=-1), dict(full=2), dict(full=-1),
        dict(planes=(None, p, None)), dict(planes=(p, None, None)),
        dict(planes=three), dict(layout=1, planes=three), dict(layout=3, planes=three),                    # V plane, semi-planar
        dict(layout=2), dict(layout=4),                                                                    # no V plane, planar
        dict(row=(8, 32, 0)), dict(row=(32, 9, 0)), dict(layout=1, row=(32, 9, 0)),                        # W = 9: 9, 10 bytes
        dict(layout=2, planes=three, row=(8, 32, 32)), dict(layout=2, planes=three, row=(32, 4, 32)), dict(layout=2, planes=three, row=(32, 32, 4)),
        dict(layout=3, row=(16, 32, 0)), dict(layout=3, row=(32, 18, 0)),                                  # 18, 20 bytes
        dict(layout=4, planes=three, row=(16, 32, 32)), dict(layout=4, planes=three, row=(32, 8, 32)), dict(layout=4, planes=three, row=(32, 32, 8)),
        dict(img=(-4, 0, 0)), dict(img=(0, -4, 0)), dict(layout=2, planes=three, img=(0, 0, -4)),
        dict(B=0), dict(H=0), dict(W=0), dict(W=-3),
        dict(layout=3, planes=(p + 1, p + 1024, None)), dict(layout=3, planes=(p, p + 1025, None)),        # 16-bit: odd anything
        dict(layout=3, row=(33, 32, 0)), dict(layout=3, row=(32, 33, 0)), dict(layout=3, img=(1, 0, 0)), dict(layout=3, img=(0, 511, 0)),
        dict(layout=4, planes=(p, p + 1024, p + 2049)), dict(layout=4, planes=three, row=(32, 32, 33)), dict(layout=4, planes=three, img=(0, 0, 3)),
    ]
    for k in refused:
        assert rgb(**k) == bad, k
        assert fused(**k) == bad, k
    assert rgb(dst=False) == bad and rgb(dr=3 * W - 1) == bad and rgb(di=-1) == bad
    assert fused(out=False) == bad and fused(Hp=0) == bad and fused(Wp=W - 1) == bad
    torch.cuda.synchronize()
    assert bool((rgb_out == 0x5A).all()) and bool((f32_out == -7.0).all()) and bool((u8 == 77).all())
    for k in (dict(), dict(layout=1), dict(layout=2, planes=three), dict(layout=3), dict(layout=4, planes=three)):   # and the accepted ones write
        rgb_out.fill_(0x5A)
        f32_out.fill_(-7.0)
        assert rgb(**k) == 0 and fused(**k) == 0, k
        torch.cuda.synchronize()
        assert not bool((rgb_out == 0x5A).any()) and not bool((f32_out == -7.0).any())


def test_predict_frames_yuv_equals_predict_frames(detector):  # noqa: F811
    det = detector
    kw = dict(input_size=128, conf_thres=0.001)
    y, uv = _synthetic_nv12(3, 90, 120, seed=40)
    rgb = _nv12_ref.nv12_to_rgb(y, uv)
    want = det.predict_frames(rgb, **kw)
    assert sum(len(d) for d in want) > 0 and all(d.img_hw == (90, 120) for d in want)
    host = {layout: ref.from_nv12(y, uv, layout, seed=3) for layout in ('i420', 'yv12', 'nv21', 'p010', 'i010')}
    for layout, planes in host.items():
        assert np.array_equal(ref.to_rgb(planes, layout), rgb)
        _same(det.predict_frames_yuv(planes, layout, **kw), want)                                          # host numpy planes
    _same(det.predict_frames_yuv(tuple(_dev(a) for a in host['i420']), 'i420', **kw), want)                # separate device planes
    _same(det.predict_frames_yuv(tuple(_dev(a) for a in host['p010']), 'p010', **kw), want)
    _same(det.predict_frames_yuv(tuple(torch.from_numpy(a[1]) for a in host['yv12']), 'yv12', **kw), want[1:2])   # 2-d planes: one frame
    for layout in ('yv12', 'i010', 'nv21'):                                                                # a single host surface
        surface = np.concatenate([a.reshape(3, -1) for a in host[layout]], axis=1).reshape(3, 135, 120)
        _same(det.predict_frames_yuv(surface, layout, **kw), want)
    _same(det.predict_frames_yuv(_dev(surface[1]), 'nv21', **kw), want[1:2])                               # one 2-d device surface
    want709 = det.predict_frames(_nv12_ref.nv12_to_rgb(y, uv, 'bt709', True), **kw)
    assert not np.array_equal(_nv12_ref.nv12_to_rgb(y, uv, 'bt709', True), rgb)
    _same(det.predict_frames_yuv(host['i010'], 'i010', matrix='bt709', full_range=True, **kw), want709)
    rows = det.frames_yuv_to_json(host['i420'], 'i420', [7, 8, 9], **kw)
    assert rows == det.frames_to_json(rgb, [7, 8, 9], **kw) and len(rows) == sum(len(d) for d in want)
    assert det.frames_yuv_to_json(_dev(surface), 'nv21', [7, 8, 9], **kw) == rows
    _same(det.predict_frames_yuv((y, uv), 'nv12', **kw), det.predict_frames_nv12(y, uv, **kw))
