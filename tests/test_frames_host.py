"""CPU tests of the video-frame input path: the C ABI of mydet_frames_to_input_f32 (exported, declared, bound, argument
checks before any launch), Detector.predict_frames' input validation on a meta-device model, and that the PIL path keeps
its surface."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = 'mydet_frames_to_input_f32'


def _header():
    return open(os.path.join(ROOT, 'include', 'mydet.h')).read()


def test_entry_point_is_exported_declared_and_bound():
    from mydetection_amd import _lib
    header = _header()
    assert re.search(r'\bint\s+' + NAME + r'\s*\(', header)
    assert NAME in _lib.SIGNATURES and len(_lib.SIGNATURES[NAME]) == 23
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), NAME)
    assert _lib.lib().mydet_frames_to_input_f32.argtypes == _lib.SIGNATURES[NAME]
    limit = int(re.search(r'#define MYDET_FRAMES_MAX_TAPS\s+(\d+)', header).group(1))
    assert limit == _lib.FRAMES_MAX_TAPS and limit % 2 == 1 and limit >= 7      # Pillow's ksize is odd; 1080p -> 360 rows has 7 taps


def test_abi_argument_checks():
    """Every call below must fail before touching its (host) pointers."""
    from mydetection_amd import _lib
    lib = _lib.lib()
    buf = (ctypes.c_float * 256)()
    p = (ctypes.cast(buf, ctypes.c_void_p).value + 15) // 16 * 16
    mean = (ctypes.c_float * 3)(0.485, 0.456, 0.406)
    std = (ctypes.c_float * 3)(0.229, 0.224, 0.225)
    limit = _lib.FRAMES_MAX_TAPS

    def call(src=p, B=1, H=8, W=8, img=192, row=24, out=p, Hp=8, Wp=8, oh=4, ow=4, top=0, left=0, bx=p, kx=p, ksx=5, by=p, ky=p,
             ksy=5, norm=0, mean=mean, std=std):
        return lib.mydet_frames_to_input_f32(src, B, H, W, img, row, out, Hp, Wp, oh, ow, top, left, bx, kx, ksx, by, ky, ksy, norm,
                                             mean, std, None)
    bad = -1
    assert call(src=None) == bad and call(out=None) == bad
    assert call(B=0) == bad and call(B=-1) == bad
    assert call(H=0) == bad and call(W=-3) == bad and call(Hp=0) == bad and call(Wp=0) == bad and call(oh=0) == bad and call(ow=0) == bad
    assert call(top=-1) == bad and call(left=-1) == bad
    assert call(row=23) == bad and call(img=-192) == bad                        # rows overlap / negative frame stride
    assert call(top=5) == bad and call(left=5) == bad and call(oh=9) == bad and call(ow=9) == bad       # the window overruns Hp x Wp
    assert call(Hp=3) == bad and call(Wp=3) == bad
    assert call(ksy=limit + 1) == bad and call(ksx=limit + 1) == bad and call(ksy=0) == bad and call(ksx=0) == bad
    assert call(bx=None) == bad and call(kx=None) == bad and call(by=None) == bad and call(ky=None) == bad   # half a table
    assert call(bx=None, kx=None) == bad and call(by=None, ky=None) == bad      # no table, but the size changes
    assert call(norm=1, mean=None) == bad and call(norm=1, std=None) == bad


def _meta_detector():
    from mydetection_amd.api import Detector
    from mydetection_amd.models.general import name_to_model
    with torch.device('meta'):
        m, cfg = name_to_model('yolov3_80')
    return Detector(model_and_cfg=(m.eval(), cfg))


def test_predict_frames_rejects_bad_input_before_any_gpu_work():
    det = _meta_detector()
    assert next(det.model.parameters()).device.type == 'meta'
    with pytest.raises(TypeError, match='float32'):
        det.predict_frames(np.zeros((2, 8, 8, 3), np.float32))
    with pytest.raises(TypeError, match='float32'):
        det.predict_frames(torch.zeros(8, 8, 3))
    with pytest.raises(ValueError, match=r'\(8, 8, 4\)'):
        det.predict_frames(np.zeros((8, 8, 4), np.uint8))
    with pytest.raises(ValueError, match=r'\(8, 8\)'):
        det.predict_frames(torch.zeros(8, 8, dtype=torch.uint8))
    with pytest.raises(ValueError, match=r'\(0, 8, 8, 3\)'):
        det.predict_frames(np.zeros((0, 8, 8, 3), np.uint8))
    with pytest.raises(TypeError, match='str'):
        det.predict_frames(['frame.png'])
    with pytest.raises(TypeError, match='int64'):                               # the bad frame of a list
        det.frames_to_json([np.zeros((8, 8, 3), np.uint8), np.zeros((8, 8, 3), np.int64)], [0, 1])


def test_frame_groups_by_size_in_input_order():
    from mydetection_amd.api import Detector
    a, b = np.zeros((2, 6, 8, 3), np.uint8), torch.ones(8, 6, 3, dtype=torch.uint8)
    c = np.full((6, 8, 3), 2, np.uint8)[:, ::-1]                                # a negative stride: copied on the host
    n, groups = Detector._frame_groups([a, b, c])
    assert n == 4 and [g[0] for g in groups] == [[0, 1, 3], [2]]
    assert [tuple(t.shape) for t in groups[0][1]] == [(2, 6, 8, 3), (1, 6, 8, 3)] and tuple(groups[1][1][0].shape) == (1, 8, 6, 3)
    assert all(t.dtype == torch.uint8 for g in groups for t in g[1])
    n, groups = Detector._frame_groups(torch.zeros(5, 4, 4, 3, dtype=torch.uint8))
    assert n == 5 and groups[0][0] == [0, 1, 2, 3, 4]


def test_frames_to_input_has_no_cpu_path():
    from mydetection_amd import ops
    geo = (None, (0, 0), (32, 32), None)
    with pytest.raises(RuntimeError):
        ops.frames_to_input(torch.zeros(1, 20, 20, 3, dtype=torch.uint8), geo, 'RGB_1')


def test_the_pil_path_keeps_its_surface():
    from mydetection_amd.api import Detector
    assert str(inspect.signature(Detector.predict_batch)) == '(self, pil_imgs, **kwargs)'
    assert str(inspect.signature(Detector.preprocess_batch)) == '(self, pil_imgs, **kwargs)'
    assert str(inspect.signature(Detector.predict_frames)) == '(self, frames, **kwargs)'
    assert str(inspect.signature(Detector.frames_to_json)) == "(self, frames, img_ids, eval_type='x1y1wh', catIdx2id=None, **kwargs)"
    det = _meta_detector()
    with pytest.raises(AssertionError, match='PIL.Image'):
        next(det.preprocess_batch([np.zeros((8, 8, 3), np.uint8)], input_size=32))
    with pytest.raises(AssertionError, match='PIL.Image'):
        det.predict_batch([torch.zeros(8, 8, 3, dtype=torch.uint8)], input_size=32)
