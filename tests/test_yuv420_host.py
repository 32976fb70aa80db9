"""CPU tests of the 4:2:0 input path: the numpy helper (_yuv420_ref) against itself, the C ABI of mydet_yuv420_to_rgb_u8 /
mydet_yuv420_to_input_f32 (declared, exported, bound; the ABI version unchanged), and the argument handling of ops.yuv420_* and
Detector.predict_frames_yuv with no device present."""
import ctypes
import re

import numpy as np
import pytest
import torch

import _nv12_ref
import _yuv420_ref as ref
from test_frames_host import _header, _meta_detector

NAMES = ('mydet_yuv420_to_rgb_u8', 'mydet_yuv420_to_input_f32')
SELECTORS = ('MYDET_YUV420_NV12', 'MYDET_YUV420_NV21', 'MYDET_YUV420_I420', 'MYDET_YUV420_P010', 'MYDET_YUV420_I010')
GEO = (None, (0, 0), (32, 32), None)


def _planes(*a, **k):
    from mydetection_amd.api import Detector
    return Detector._yuv_planes(*a, **k)


def test_reduction_rule():
    assert ref.reduce10([64, 512, 940, 1021, 1022, 1023]).tolist() == [16, 128, 235, 255, 255, 255]
    assert ref.reduce10([0, 1, 2, 1017, 1018]).tolist() == [0, 0, 1, 254, 255]


@pytest.mark.parametrize('matrix,full_range', list(_nv12_ref.TABLE))
def test_i420_equals_direct_nearest_neighbour_indexing(matrix, full_range):
    y, u, v = ref.random_planes('i420', 2, 9, 11, seed=3)
    got = ref.to_rgb((y, u, v), 'i420', matrix, full_range)
    cy, crv, cgu, cgv, cbu = _nv12_ref.TABLE[(matrix, full_range)]
    for b, r, c in [(0, 0, 0), (1, 8, 10), (0, 3, 7), (1, 5, 2), (0, 8, 9), (1, 0, 10)]:
        C = int(y[b, r, c]) - (0 if full_range else 16)
        D, E = int(u[b, r >> 1, c >> 1]) - 128, int(v[b, r >> 1, c >> 1]) - 128
        want = [min(255, max(0, t >> 8)) for t in (cy * C + crv * E + 128, cy * C - cgu * D - cgv * E + 128, cy * C + cbu * D + 128)]
        assert got[b, r, c].tolist() == want
    assert np.array_equal(ref.to_rgb((y, v, u), 'yv12', matrix, full_range), got)
    assert np.array_equal(ref.to_rgb((y, np.stack([v, u], -1)), 'nv21', matrix, full_range), got)


def test_p010_and_i010_of_the_same_values_give_the_same_planes():
    rng = np.random.Generator(np.random.PCG64(5))
    y, u, v = (rng.integers(0, 1024, size=s) for s in ((2, 7, 9), (2, 4, 5), (2, 4, 5)))
    p = ref.from_values10(y, u, v, 'p010', rng)
    i = ref.from_values10(y, u, v, 'i010', rng)
    assert p[0].dtype == i[0].dtype == np.uint16 and (p[0] & 63).any() and (i[0] >> 10).any()      # ignored bits are set
    (py, puv), (iy, iuv) = ref.to_nv12(p, 'p010'), ref.to_nv12(i, 'i010')
    assert np.array_equal(py, iy) and np.array_equal(puv, iuv)
    assert np.array_equal(py, ref.reduce10(y)) and np.array_equal(puv[..., 1], ref.reduce10(v))


@pytest.mark.parametrize('layout', ref.LAYOUTS)
def test_clip_frames_are_the_nv12_clip_frame(layout):
    y, uv = _nv12_ref.clip_frame()
    gy, guv = ref.to_nv12(ref.clip_frame(layout), layout)
    assert np.array_equal(gy, y) and np.array_equal(guv, uv)
    if layout in ref.WORDS:
        words = ref.clip_frame(layout)[0]
        v10 = words >> 6 if layout == 'p010' else words & 1023
        assert {1021, 1022, 1023} <= set(np.unique(v10).tolist())
        assert ((words & 63) if layout == 'p010' else (words >> 10)).any()


@pytest.mark.parametrize('layout', ref.LAYOUTS)
def test_planes_from_nv12_repack_to_the_same_nv12(layout):
    y, uv = _nv12_ref.random_nv12(2, 7, 9, seed=1)
    planes = ref.from_nv12(y, uv, layout, seed=2)                                # asserts the round trip itself
    assert len(planes) == (3 if layout in ref.PLANAR else 2) and planes[0].dtype == (np.uint16 if layout in ref.WORDS else np.uint8)
    assert np.array_equal(ref.to_rgb(planes, layout, 'bt709', True), _nv12_ref.nv12_to_rgb(y, uv, 'bt709', True))


def test_entry_points_are_declared_exported_and_bound():
    from mydetection_amd import _lib
    header = _header()
    dll = ctypes.CDLL(_lib.LIB_PATH)
    for name, nargs in zip(NAMES, (8, 21)):
        assert re.search(r'\bint\s+' + name + r'\s*\(', header)
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name]) == nargs
        assert hasattr(dll, name)
        assert getattr(_lib.lib(), name).argtypes == _lib.SIGNATURES[name]
    for value, name in enumerate(SELECTORS):
        assert re.search(r'#define\s+' + name + r'\s+' + str(value) + r'\b', header)
        assert getattr(_lib, name[len('MYDET_'):]) == value
    assert 'typedef struct mydet_yuv420_src' in header
    assert re.search(r'#define\s+MYDET_ABI_VERSION\s+2\b', header) and _lib.ABI_VERSION == 2 and _lib.lib().mydet_abi_version() == 2
    s = _lib.Yuv420Src
    assert ctypes.sizeof(s) == 3 * 8 + 6 * 8 + 4 * 4 and s.layout.offset == 72 and s.row_bytes.offset == 48
    assert re.search(r'min\(255, \(v10 \+ 2\) >> 2\)', header)


def test_abi_argument_checks_on_host_pointers():
    """Every call below must fail before touching its (host) pointers."""
    from mydetection_amd import _lib
    lib = _lib.lib()
    buf = (ctypes.c_float * 256)()
    p = (ctypes.cast(buf, ctypes.c_void_p).value + 15) // 16 * 16

    def rgb(layout=0, planes=(p, p, None), img=(72, 50, 0), row=(9, 10, 0), matrix=0, full=0, B=1, H=8, W=9, dst=p, di=216, dr=27, null=False):
        src = _lib.Yuv420Src((ctypes.c_void_p * 3)(*planes), (ctypes.c_int64 * 3)(*img), (ctypes.c_int64 * 3)(*row), layout, matrix, full, 0)
        return lib.mydet_yuv420_to_rgb_u8(None if null else ctypes.byref(src), B, H, W, dst, di, dr, None)
    bad = -1
    assert rgb(null=True) == bad and rgb(layout=5) == bad and rgb(layout=-1) == bad and rgb(matrix=2) == bad and rgb(full=-1) == bad
    assert rgb(planes=(None, p, None)) == bad and rgb(planes=(p, None, None)) == bad
    assert rgb(planes=(p, p, p)) == bad and rgb(layout=2, row=(9, 5, 5)) == bad and rgb(layout=4, row=(18, 10, 10)) == bad     # plane[2]
    assert rgb(row=(8, 10, 0)) == bad and rgb(row=(9, 9, 0)) == bad and rgb(layout=1, row=(9, 9, 0)) == bad
    assert rgb(layout=2, planes=(p, p, p), row=(9, 4, 5)) == bad and rgb(layout=2, planes=(p, p, p), row=(9, 5, 4)) == bad
    assert rgb(layout=3, row=(17, 20, 0)) == bad and rgb(layout=3, row=(18, 19, 0)) == bad and rgb(layout=3, row=(16, 20, 0)) == bad
    assert rgb(layout=4, planes=(p, p, p), row=(18, 8, 10)) == bad
    assert rgb(img=(-1, 50, 0)) == bad and rgb(img=(72, -1, 0)) == bad and rgb(layout=2, planes=(p, p, p), row=(9, 5, 5), img=(72, 20, -1)) == bad
    assert rgb(B=0) == bad and rgb(H=0) == bad and rgb(W=-1) == bad and rgb(dst=None) == bad and rgb(dr=26) == bad
    assert rgb(layout=3, planes=(p + 1, p, None), row=(18, 20, 0)) == bad and rgb(layout=3, planes=(p, p + 1, None), row=(18, 20, 0)) == bad
    assert rgb(layout=3, row=(18, 21, 0)) == bad and rgb(layout=3, row=(18, 20, 0), img=(145, 100, 0)) == bad
    assert rgb(layout=4, planes=(p, p, p + 1), row=(18, 10, 10)) == bad and rgb(layout=4, planes=(p, p, p), row=(18, 10, 11)) == bad


def test_names_are_checked_before_any_device_is_touched():
    from mydetection_amd import ops
    y, uv = torch.zeros(1, 8, 8, dtype=torch.uint8), torch.zeros(1, 4, 4, 2, dtype=torch.uint8)
    with pytest.raises(ValueError, match='nv16'):
        ops.yuv420_to_rgb((y, uv), 'nv16')
    with pytest.raises(ValueError, match='NV12'):
        ops.yuv420_to_input((y, uv), 'NV12', GEO, 'RGB_1')
    with pytest.raises(ValueError, match='bt2020'):
        ops.yuv420_to_rgb((y, uv), 'nv12', matrix='bt2020')
    with pytest.raises(ValueError, match='BT601'):
        ops.yuv420_to_input((y, uv), 'nv21', GEO, 'RGB_1', matrix='BT601')
    det = _meta_detector()
    with pytest.raises(ValueError, match='yuv444'):
        det.predict_frames_yuv(np.zeros((12, 8), np.uint8), 'yuv444')
    with pytest.raises(ValueError, match='rec709'):
        det.predict_frames_yuv(np.zeros((12, 8), np.uint8), 'i420', matrix='rec709')
    with pytest.raises(ValueError, match='rec709'):
        det.frames_yuv_to_json((y, uv), 'nv12', [0], matrix='rec709')


def test_ops_reject_wrong_types_dtypes_and_shapes():
    from mydetection_amd import ops
    u8 = lambda *s: torch.zeros(s, dtype=torch.uint8)
    i16 = lambda *s: torch.zeros(s, dtype=torch.int16)
    for call in (lambda pl, lay: ops.yuv420_to_rgb(pl, lay), lambda pl, lay: ops.yuv420_to_input(pl, lay, GEO, 'RGB_1')):
        with pytest.raises(TypeError, match='int16'):
            call((u8(1, 8, 8), i16(1, 4, 4, 2)), 'nv12')
        with pytest.raises(TypeError, match='uint8'):
            call((u8(1, 8, 8), u8(1, 4, 4, 2)), 'p010')
        with pytest.raises(TypeError, match='float32'):
            call((i16(1, 8, 8), i16(1, 4, 4), torch.zeros(1, 4, 4)), 'i010')
        with pytest.raises(TypeError, match='ndarray'):
            call((np.zeros((1, 8, 8), np.uint8), u8(1, 4, 4, 2)), 'nv12')
        with pytest.raises(TypeError, match='Tensor'):
            call(u8(1, 12, 8), 'nv12')
        with pytest.raises(ValueError, match=r'\(y, u, v\)'):
            call((u8(1, 8, 8), u8(1, 4, 4, 2)), 'i420')
        with pytest.raises(ValueError, match=r'\(y, uv\)'):
            call((u8(1, 8, 8), u8(1, 4, 4), u8(1, 4, 4)), 'nv21')
        with pytest.raises(ValueError, match=r'\(2, 5, 5, 2\) expected'):
            call((u8(2, 9, 10), u8(2, 4, 5, 2)), 'nv21')
        with pytest.raises(ValueError, match=r'\(2, 5, 5\) expected'):
            call((u8(2, 9, 10), u8(2, 5, 5), u8(2, 5, 4)), 'yv12')
        with pytest.raises(ValueError, match=r'\(2, 5, 5\) expected'):
            call((i16(2, 9, 10), i16(2, 5, 5, 2), i16(2, 5, 5)), 'i010')
        with pytest.raises(ValueError, match=r'\(2, 5, 5, 2\) expected'):
            call((i16(2, 9, 10), i16(2, 5, 5)), 'p010')
        with pytest.raises(ValueError, match=r'\(8,\)'):
            call((u8(8), u8(4, 2)), 'nv12')
        with pytest.raises(RuntimeError):                                        # all well, but on the host: no CPU path
            call((i16(1, 8, 8), i16(1, 4, 4), i16(1, 4, 4)), 'i010')
    if hasattr(torch, 'uint16'):
        with pytest.raises(RuntimeError):
            ops.yuv420_to_rgb((torch.zeros(8, 8, dtype=torch.uint16), torch.zeros(4, 4, 2, dtype=torch.uint16)), 'p010')


def test_detector_planes_reject_wrong_types_dtypes_and_shapes():
    det = _meta_detector()
    with pytest.raises(TypeError, match='float32'):
        det.predict_frames_yuv(np.zeros((12, 8), np.float32), 'i420')
    with pytest.raises(TypeError, match='uint8'):
        det.predict_frames_yuv((np.zeros((8, 8), np.uint8), np.zeros((4, 4, 2), np.uint8)), 'p010')
    with pytest.raises(TypeError, match='uint16'):
        _planes((np.zeros((8, 8), np.uint16), np.zeros((4, 4, 2), np.uint16)), 'nv21')
    with pytest.raises(TypeError, match='int32'):
        _planes((torch.zeros(8, 8, dtype=torch.int32),) * 3, 'i010')
    with pytest.raises(TypeError, match='str'):
        _planes('frame.yuv', 'i420')
    with pytest.raises(TypeError, match='list'):
        _planes((np.zeros((8, 8), np.uint8), [1, 2], [3]), 'i420')
    with pytest.raises(ValueError, match=r'\(y, u, v\)'):
        _planes((np.zeros((8, 8), np.uint8), np.zeros((4, 4, 2), np.uint8)), 'yv12')
    with pytest.raises(ValueError, match=r'\(1, 4, 4\) expected'):
        _planes((np.zeros((8, 8), np.uint8), np.zeros((4, 4), np.uint8), np.zeros((4, 3), np.uint8)), 'i420')
    with pytest.raises(ValueError, match=r'\(2, 5, 5, 2\) expected'):
        det.predict_frames_yuv((np.zeros((2, 9, 10), np.uint16), np.zeros((2, 5, 5), np.uint16)), 'p010')
    for bad_surface in (np.zeros((2, 13, 8), np.uint8), np.zeros((14, 8), np.uint8), np.zeros((2, 12, 7), np.uint8), np.zeros((8, 8), np.uint8)):
        for layout in ('nv21', 'i420'):                                          # rows != 3H/2, odd H (9 + 5 rows), odd W
            with pytest.raises(ValueError, match='single .* surface'):
                _planes(bad_surface, layout)
    with pytest.raises(ValueError, match='single .* surface'):
        det.predict_frames_yuv(np.zeros((13, 8), np.uint16), 'i010')


def test_separate_planes_pass_through():
    y, u, v = torch.zeros(2, 9, 11, dtype=torch.uint8), np.ones((2, 5, 6), np.uint8), torch.full((2, 5, 6), 2, dtype=torch.uint8)
    py, pu, pv = _planes((y, u, v), 'i420')
    assert py is y and pv is v and tuple(pu.shape) == (2, 5, 6) and int(pu.min()) == 1
    py, pu, pv = _planes((y[0], u[0], v[0]), 'yv12')                             # 2-d: one frame; storage order is kept
    assert tuple(py.shape) == (1, 9, 11) and tuple(pu.shape) == tuple(pv.shape) == (1, 5, 6) and py.data_ptr() == y.data_ptr()
    assert int(pu.max()) == 1 and int(pv.min()) == 2
    w = np.full((9, 11), 0xFFC0, np.uint16)                                      # numpy words cross as int16: the same bits
    py, puv = _planes((w, np.zeros((5, 6, 2), np.uint16)), 'p010')
    assert py.dtype == torch.int16 and tuple(py.shape) == (1, 9, 11) and tuple(puv.shape) == (1, 5, 6, 2) and int(py[0, 0, 0]) == -64


def test_single_surface_is_split_into_views():
    s = torch.arange(2 * 12 * 6, dtype=torch.int64).to(torch.uint8).view(2, 12, 6)
    y, uv = _planes(s, 'nv21')
    assert tuple(y.shape) == (2, 8, 6) and tuple(uv.shape) == (2, 4, 3, 2)
    assert y.data_ptr() == s.data_ptr() and uv.data_ptr() == s.data_ptr() + 8 * 6 and uv.stride() == (72, 6, 2, 1)
    for layout in ('i420', 'yv12'):
        y, c1, c2 = _planes(s, layout)
        assert tuple(y.shape) == (2, 8, 6) and tuple(c1.shape) == tuple(c2.shape) == (2, 4, 3)
        assert y.data_ptr() == s.data_ptr() and c1.data_ptr() == s.data_ptr() + 48 and c2.data_ptr() == s.data_ptr() + 60
        assert y.stride() == (72, 6, 1) and c1.stride() == c2.stride() == (72, 3, 1)
        s[1, 9, 5], s[1, 11, 0] = 201, 202                                       # writes through: the views share the storage
        assert int(c1[1, 3, 2]) == 201 and int(c2[1, 2, 0]) == 202
        assert torch.equal(c1[0].flatten(), s[0, 8:10].flatten()) and torch.equal(c2[0].flatten(), s[0, 10:].flatten())
    a = np.zeros((6, 4), np.uint16)                                              # numpy words, 2-d
    y, u, v = _planes(a, 'i010')
    assert y.dtype == torch.int16 and tuple(y.shape) == (1, 4, 4) and tuple(u.shape) == tuple(v.shape) == (1, 2, 2)
    a[5, 3], a[4, 0] = 9, 7
    assert int(v[0, 1, 1]) == 9 and int(u[0, 0, 0]) == 7
    y, uv = _planes(a, 'p010')
    assert tuple(uv.shape) == (1, 2, 2, 2) and int(uv[0, 1, 1, 1]) == 9
