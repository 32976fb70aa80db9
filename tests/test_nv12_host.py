"""CPU tests of the NV12 input path: Detector._yuv_planes for layout 'nv12' (plane splitting and validation, no device), the C ABI of
mydet_nv12_to_rgb_u8 / mydet_nv12_to_input_f32 (exported, declared, bound, argument checks before any launch), and that an
unknown matrix name is refused before any device is touched."""
import ctypes
import re

import numpy as np
import pytest
import torch

import _nv12_ref
from test_frames_host import _header, _meta_detector

NAMES = ('mydet_nv12_to_rgb_u8', 'mydet_nv12_to_input_f32')


def _planes(y, uv=None, device=None):
    from mydetection_amd.api import Detector
    return Detector._yuv_planes(y if uv is None else (y, uv), 'nv12', device)


def test_the_reference_table_is_the_rounded_matrices():
    assert _nv12_ref.table_from_matrices() == _nv12_ref.TABLE


def test_planes_reject_wrong_dtype_and_type():
    with pytest.raises(TypeError, match='float32'):
        _planes(np.zeros((2, 12, 8), np.float32))
    with pytest.raises(TypeError, match='int16'):
        _planes(torch.zeros(8, 8, dtype=torch.uint8), torch.zeros(4, 4, 2, dtype=torch.int16))
    with pytest.raises(TypeError, match='float64'):
        _planes(np.zeros((8, 8), np.uint8), np.zeros((4, 4, 2), np.float64))
    with pytest.raises(TypeError, match='str'):
        _planes('frame.nv12')
    with pytest.raises(TypeError, match='list'):
        _planes(np.zeros((8, 8), np.uint8), [1, 2])


def test_planes_reject_wrong_shapes():
    u8 = lambda *s: np.zeros(s, np.uint8)
    with pytest.raises(ValueError, match=r'\(2, 8, 8, 1\)'):                     # rank
        _planes(u8(2, 8, 8, 1), u8(2, 4, 4, 2))
    with pytest.raises(ValueError, match=r'\(8,\)'):
        _planes(torch.zeros(8, dtype=torch.uint8))
    with pytest.raises(ValueError, match=r'\(0, 12, 8\)'):
        _planes(u8(0, 12, 8))
    for bad_uv in (u8(2, 4, 4, 2), u8(2, 5, 4, 2), u8(2, 4, 5, 2), u8(2, 5, 5, 1), u8(1, 5, 5, 2), u8(5, 5, 2), u8(2, 5, 10)):
        with pytest.raises(ValueError, match=r'\(2, 5, 5, 2\) expected'):        # Y 9 x 10: ceil(9/2) x ceil(10/2) pairs
            _planes(u8(2, 9, 10), bad_uv)
    with pytest.raises(ValueError, match=r'\(1, 4, 4, 2\) expected'):
        _planes(u8(8, 8), u8(4, 4))
    for bad_surface in (u8(2, 13, 8), u8(14, 8), u8(2, 12, 7), u8(8, 8)):        # rows != 3H/2, odd H (9 + 5 rows), odd W
        with pytest.raises(ValueError, match="single 'nv12' surface"):
            _planes(bad_surface)


def test_separate_planes_pass_through():
    y, uv = torch.zeros(2, 9, 11, dtype=torch.uint8), np.ones((2, 5, 6, 2), np.uint8)
    yp, uvp = _planes(y, uv)
    assert yp is y and tuple(uvp.shape) == (2, 5, 6, 2) and uvp.dtype == torch.uint8 and int(uvp.min()) == 1
    yp, uvp = _planes(y[0], uv[0])                                               # 2-d: one frame
    assert tuple(yp.shape) == (1, 9, 11) and tuple(uvp.shape) == (1, 5, 6, 2) and yp.data_ptr() == y.data_ptr()


def test_single_surface_is_split_into_views():
    s = torch.arange(2 * 12 * 6, dtype=torch.int64).to(torch.uint8).view(2, 12, 6)
    y, uv = _planes(s)
    assert tuple(y.shape) == (2, 8, 6) and tuple(uv.shape) == (2, 4, 3, 2)
    assert y.data_ptr() == s.data_ptr() and uv.data_ptr() == s.data_ptr() + 8 * 6
    assert y.stride() == (72, 6, 1) and uv.stride() == (72, 6, 2, 1)
    s[1, 2, 3], s[1, 9, 5] = 201, 202                                            # writes through: the views share the storage
    assert int(y[1, 2, 3]) == 201 and int(uv[1, 1, 2, 1]) == 202
    assert torch.equal(uv[0, 0].flatten(), s[0, 8])
    a = np.zeros((6, 4), np.uint8)                                               # numpy, 2-d
    y, uv = _planes(a)
    assert tuple(y.shape) == (1, 4, 4) and tuple(uv.shape) == (1, 2, 2, 2)
    a[5, 3] = 9
    assert int(uv[0, 1, 1, 1]) == 9


def test_entry_points_are_exported_declared_and_bound():
    from mydetection_amd import _lib
    header = _header()
    dll = ctypes.CDLL(_lib.LIB_PATH)
    for name, nargs in zip(NAMES, (15, 28)):
        assert re.search(r'\bint\s+' + name + r'\s*\(', header)
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name]) == nargs
        assert hasattr(dll, name)
        assert getattr(_lib.lib(), name).argtypes == _lib.SIGNATURES[name]
    for row in _nv12_ref.TABLE.values():                                         # the header documents the table
        assert re.search(r'\s+'.join(str(v) for v in row), header), row


def test_abi_argument_checks():
    """Every call below must fail before touching its (host) pointers."""
    from mydetection_amd import _lib
    lib = _lib.lib()
    buf = (ctypes.c_float * 256)()
    p = (ctypes.cast(buf, ctypes.c_void_p).value + 15) // 16 * 16
    mean = (ctypes.c_float * 3)(0.485, 0.456, 0.406)
    std = (ctypes.c_float * 3)(0.229, 0.224, 0.225)
    limit = _lib.FRAMES_MAX_TAPS
    bad = -1

    def rgb(y=p, yi=72, yr=9, uv=p, ui=50, ur=10, B=1, H=8, W=9, dst=p, di=216, dr=27, matrix=0, full=0):
        return lib.mydet_nv12_to_rgb_u8(y, yi, yr, uv, ui, ur, B, H, W, dst, di, dr, matrix, full, None)
    assert rgb(y=None) == bad and rgb(uv=None) == bad and rgb(dst=None) == bad
    assert rgb(B=0) == bad and rgb(H=0) == bad and rgb(W=-1) == bad
    assert rgb(yr=8) == bad and rgb(ur=9) == bad and rgb(dr=26) == bad          # pitches below W, 2 * ceil(W / 2), 3 * W
    assert rgb(yi=-1) == bad and rgb(ui=-1) == bad and rgb(di=-1) == bad
    assert rgb(matrix=2) == bad and rgb(matrix=-1) == bad and rgb(full=2) == bad and rgb(full=-1) == bad

    def fused(y=p, yi=72, yr=9, uv=p, ui=50, ur=10, B=1, H=8, W=9, matrix=0, full=0, out=p, Hp=8, Wp=8, oh=4, ow=4, top=0, left=0,
              bx=p, kx=p, ksx=5, by=p, ky=p, ksy=5, norm=0, mean=mean, std=std):
        return lib.mydet_nv12_to_input_f32(y, yi, yr, uv, ui, ur, B, H, W, matrix, full, out, Hp, Wp, oh, ow, top, left,
                                           bx, kx, ksx, by, ky, ksy, norm, mean, std, None)
    assert fused(y=None) == bad and fused(uv=None) == bad and fused(out=None) == bad
    assert fused(B=0) == bad and fused(H=0) == bad and fused(W=0) == bad and fused(Hp=0) == bad and fused(Wp=0) == bad
    assert fused(oh=0) == bad and fused(ow=0) == bad and fused(top=-1) == bad and fused(left=-1) == bad
    assert fused(yr=8) == bad and fused(ur=9) == bad and fused(yi=-1) == bad and fused(ui=-1) == bad
    assert fused(matrix=2) == bad and fused(matrix=-1) == bad and fused(full=2) == bad and fused(full=-1) == bad
    assert fused(top=5) == bad and fused(left=5) == bad and fused(oh=9) == bad and fused(ow=9) == bad
    assert fused(ksy=limit + 1) == bad and fused(ksx=limit + 1) == bad and fused(ksy=0) == bad and fused(ksx=0) == bad
    assert fused(bx=None) == bad and fused(kx=None) == bad and fused(by=None) == bad and fused(ky=None) == bad
    assert fused(bx=None, kx=None) == bad and fused(by=None, ky=None) == bad    # no table, but the size changes
    assert fused(norm=1, mean=None) == bad and fused(norm=1, std=None) == bad


def test_unknown_matrix_is_refused_before_any_device_is_touched():
    from mydetection_amd import ops
    y, uv = torch.zeros(1, 8, 8, dtype=torch.uint8), torch.zeros(1, 4, 4, 2, dtype=torch.uint8)
    geo = (None, (0, 0), (32, 32), None)
    with pytest.raises(ValueError, match='bt2020'):                              # host tensors: the name is checked first
        ops.nv12_to_rgb(y, uv, matrix='bt2020')
    with pytest.raises(ValueError, match='BT601'):
        ops.nv12_to_input(y, uv, geo, 'RGB_1', matrix='BT601')
    det = _meta_detector()
    with pytest.raises(ValueError, match='rec709'):
        det.predict_frames_nv12(np.zeros((12, 8), np.uint8), matrix='rec709')
    with pytest.raises(ValueError, match='rec709'):
        det.frames_nv12_to_json(y, uv, [0], matrix='rec709')
    with pytest.raises(TypeError, match='float32'):                              # and bad planes, on a meta-device model
        det.predict_frames_nv12(np.zeros((12, 8), np.float32))
    with pytest.raises(ValueError, match="single 'nv12' surface"):
        det.predict_frames_nv12(np.zeros((13, 8), np.uint8))


def test_nv12_ops_have_no_cpu_path():
    from mydetection_amd import ops
    y, uv = torch.zeros(1, 8, 8, dtype=torch.uint8), torch.zeros(1, 4, 4, 2, dtype=torch.uint8)
    with pytest.raises(RuntimeError):
        ops.nv12_to_rgb(y, uv)
    with pytest.raises(RuntimeError):
        ops.nv12_to_input(y, uv, (None, (0, 0), (32, 32), None), 'RGB_1')
