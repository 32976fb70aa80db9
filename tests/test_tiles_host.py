"""CPU tests of tiled detection on large frames: the window planner ops.tile_windows, the C ABI of the merge of tile records
(declared, exported, bound, constants, argument checks before any launch), the numpy restatement tests/_tiles_ref.py on
hand-made cases, and the argument errors of Detector(..., tiles=) on a meta-device model."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import _tiles_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {'mydet_merge_tile_records_scratch_bytes': 3, 'mydet_merge_tile_records_f32': 14}

# (H, W, size, overlap, align)
CASES = {
    '150x200': (150, 200, (96, 128), 0.25, 1),
    'one_window': (64, 64, (96, 96), 0.2, 1),
    '1080p': (1080, 1920, (640, 640), 0.2, 1),
    'odd_no_overlap': (97, 131, (32, 32), 0.0, 1),
    'align2': (96, 128, (32, 64), 0.5, 2),
}


@pytest.mark.parametrize('case', list(CASES))
def test_tile_windows(case):
    from mydetection_amd import ops
    H, W, size, overlap, align = CASES[case]
    wins = ops.tile_windows(H, W, size, overlap, True, align)
    tiles = ops.tile_windows(H, W, size, overlap, False, align)
    assert all(isinstance(v, int) for win in wins for v in win)
    h, w = min(size[0], H), min(size[1], W)
    assert all(win[2:] == (h, w) for win in tiles)                               # one size
    assert all(0 <= y0 and y0 + h <= H and 0 <= x0 and x0 + w <= W for y0, x0, _, _ in tiles)
    mask = np.zeros((H, W), bool)
    for y0, x0, _, _ in tiles:
        mask[y0:y0 + h, x0:x0 + w] = True
    assert mask.all()                                                            # every pixel is covered
    assert [t[:2] for t in tiles] == sorted(set(t[:2] for t in tiles))           # row-major, no duplicates
    assert tiles[-1][:2] == (H - h, W - w) and tiles[0][:2] == (0, 0)
    ys, xs = sorted(set(t[0] for t in tiles)), sorted(set(t[1] for t in tiles))
    assert len(tiles) == len(ys) * len(xs)
    for origins, n, t in ((ys, H, h), (xs, W, w)):                               # the step rule
        step = max(align, int(np.floor(t * (1 - overlap))) // align * align)
        assert origins[:-1] == list(range(0, n - t, step)) and origins[-1] == n - t
    if len(tiles) > 1:
        assert wins == tiles + [(0, 0, H, W)]                                    # the full frame comes last ...
    else:
        assert wins == tiles == [(0, 0, h, w)]                                   # ... and only beside more than one tile
    if align == 2:
        assert all(v % 2 == 0 for win in wins for v in win)
    if case == '150x200':
        assert wins == [(0, 0, 96, 128), (0, 72, 96, 128), (54, 0, 96, 128), (54, 72, 96, 128), (0, 0, 150, 200)]
    if case == '1080p':
        assert [t[:2] for t in tiles] == [(y, x) for y in (0, 440) for x in (0, 512, 1024, 1280)] and len(wins) == 9
    if case == 'odd_no_overlap':
        assert ys == [0, 32, 64, 65] and xs == [0, 32, 64, 96, 99]
    if case == 'align2':
        assert ys == [0, 16, 32, 48, 64] and xs == [0, 32, 64]


def test_tile_windows_errors():
    from mydetection_amd import _lib, ops
    assert ops.tile_windows(64, 64, 32, 0.5) == ops.tile_windows(64, 64, (32, 32), 0.5)
    for overlap in (-0.1, 1.0, 1.5):
        with pytest.raises(ValueError, match='overlap'):
            ops.tile_windows(100, 100, (32, 32), overlap)
    for size in ((0, 32), (32, -1)):
        with pytest.raises(ValueError, match='positive'):
            ops.tile_windows(100, 100, size)
    for H, W, size in ((97, 128, (32, 64)), (96, 131, (32, 64)), (96, 128, (33, 64)), (96, 128, (32, 63))):
        with pytest.raises(ValueError, match='align'):
            ops.tile_windows(H, W, size, 0.5, True, 2)
    assert len(ops.tile_windows(256, 256, (32, 32), 0.0, False)) == 64 == _lib.TILES_MAX
    with pytest.raises(ValueError, match='65 windows'):
        ops.tile_windows(256, 256, (32, 32), 0.0, True)
    with pytest.raises(ValueError, match='windows'):
        ops.tile_windows(1080, 1920, (64, 64))


def test_entry_points_are_declared_exported_and_bound():
    from mydetection_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'mydet.h')).read()
    assert re.search(r'\bint64_t\s+mydet_merge_tile_records_scratch_bytes\s*\(', header)
    assert re.search(r'\bint\s+mydet_merge_tile_records_f32\s*\(', header)
    handle = ctypes.CDLL(_lib.LIB_PATH)
    lib = _lib.lib()
    for name, nargs in NAMES.items():
        assert hasattr(handle, name), name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name]) == nargs
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name]
    assert lib.mydet_merge_tile_records_scratch_bytes.restype == ctypes.c_int64

    def define(name):
        return int(re.search(r'#define ' + name + r'\s+(-?\d+)', header).group(1))
    assert define('MYDET_TILES_MAX') == _lib.TILES_MAX == 64
    assert (define('MYDET_MERGE_IOU'), define('MYDET_MERGE_IOS')) == (_lib.MERGE_IOU, _lib.MERGE_IOS) == (0, 1)
    assert define('MYDET_ABI_VERSION') == _lib.ABI_VERSION == lib.mydet_abi_version() == 2
    bad_class = int(re.search(r'#define MYDET_COUNT_BAD_CLASS\s+\((-?\d+)\)', header).group(1))
    assert (ref.REC_WORDS, ref.REC_ROT_WORDS, ref.TOPK, ref.BAD_CLASS) == (_lib.REC_WORDS, _lib.REC_ROT_WORDS, _lib.REC_TOPK, bad_class)


def test_abi_argument_checks():
    """Every call below must fail before any launch: the pointers are host addresses."""
    from mydetection_amd import _lib
    lib = _lib.lib()
    size = lib.mydet_merge_tile_records_scratch_bytes
    assert size(2, 3, 4) == 2 * 3 * 512 * (16 + 8 + 4 + 8) and size(2, 3, 5) == 2 * 3 * 512 * (20 + 8 + 4 + 8)
    assert size(0, 3, 4) == size(2, 0, 4) == size(2, 65, 4) == size(2, 3, 3) == 0 and size(1, 64, 5) > 0
    buf = (ctypes.c_int32 * 64)()
    p = (ctypes.cast(buf, ctypes.c_void_p).value + 15) // 16 * 16
    W4, W5 = _lib.REC_WORDS, _lib.REC_ROT_WORDS

    def call(rec=p, ts=None, fs=None, B=2, T=3, bw=4, org=p, nms=0.5, metric=0, rot=0, out=p, scratch=p, nbytes=None):
        words = W5 if bw == 5 else W4
        ts = B * words if ts is None else ts
        fs = words if fs is None else fs
        nbytes = size(B, T, bw) if nbytes is None else nbytes
        return lib.mydet_merge_tile_records_f32(rec, ts, fs, B, T, bw, org, nms, metric, rot, out, scratch, nbytes, None)
    bad, unsupp = -1, -2
    assert call(B=0, nbytes=1 << 30) == bad and call(B=-1, nbytes=1 << 30) == bad
    assert call(T=0, nbytes=1 << 30) == bad and call(T=65, nbytes=1 << 30) == bad
    assert call(bw=3, nbytes=1 << 30) == bad and call(bw=6, nbytes=1 << 30) == bad
    assert call(metric=2) == bad and call(metric=-1) == bad
    assert call(rot=1) == bad                                                    # the rotated test needs the angle plane
    assert call(rec=None) == bad and call(org=None) == bad and call(out=None) == bad and call(scratch=None) == bad
    assert call(rec=p + 4) == bad and call(out=p + 8) == bad and call(scratch=p + 8) == bad and call(org=p + 2) == bad
    assert call(ts=2 * W4 + 2) == bad and call(fs=W4 + 1) == bad and call(ts=-2 * W4) == bad and call(fs=-W4) == bad
    assert call(nbytes=size(2, 3, 4) - 1) == bad and call(bw=5, nbytes=size(2, 3, 4)) == bad and call(nbytes=0) == bad
    assert call(bw=5, metric=1, rot=1) == unsupp


def _record(boxes, scores, cats):
    """One record with len(boxes) detections (and poison behind them, which no merge may read)."""
    n = len(boxes)
    b = np.full((512, len(boxes[0])), 7.0, np.float32)
    s = np.full(512, 2.0, np.float32)
    c = np.full(512, 1, np.int64)
    b[:n], s[:n], c[:n] = boxes, scores, cats
    return b, s, c, n


def test_reference_merge_on_hand_made_cases():
    """tests/_tiles_ref.py itself: a box and its seam-truncated half from two windows."""
    whole = _record([[60, 50, 40, 20]], [0.9], [0])                              # window 0 at (0, 0): x 40..80
    half = _record([[10, 50, 20, 20]], [0.8], [0])                               # window 1 at (60, 0): x 60..80 of the frame
    fields = [np.stack(f) for f in zip(whole[:3], half[:3])]
    counts, origins = [1, 1], [(0, 0), (60, 0)]
    cb, cc, cs = ref.candidates(*fields, counts, origins)
    assert cb[512].tolist() == [70, 50, 20, 20] and np.isnan(cs[1]) and np.isnan(cs[513]) and cs[512] == np.float32(0.8)
    iou = ref.chk.aligned_iou_matrix(cb[[0, 512]], cb[[0, 512]])[0, 1]
    ios = ref.ios_matrix(cb[[0, 512]], cb[[0, 512]])[0, 1]
    assert abs(iou - 0.5) < 1e-12 and abs(ios - 1.0) < 1e-12
    assert ref.merge_frame(*fields, counts, origins, 0.6, 'iou')[0].tolist() == [0, 512]
    assert ref.merge_frame(*fields, counts, origins, 0.6, 'ios')[0].tolist() == [0]
    assert ref.merge_frame(*fields, [1, 0], origins, 0.6, 'ios')[0].tolist() == [0]
    assert ref.merge_frame(*fields, [1, -1], origins, 0.6, 'ios')[0] is None
    fields[1][1, 0] = 0.9                                                        # equal scores: the earlier window wins
    assert ref.merge_frame(*fields, counts, origins, 0.6, 'ios')[0].tolist() == [0]
    assert ref.merge_frame(*fields, counts, [(60, 0), (0, 0)], 0.6, 'iou')[0].tolist() == [0, 512]
    fields[2][1, 0] = 3                                                          # another class: output order is class ascending
    assert ref.merge_frame(*fields, counts, origins, 0.6, 'ios')[0].tolist() == [0, 512]
    zero = np.zeros((2, 512, 4), np.float32)
    zero[:, 0] = (5, 5, 0, 10)
    assert ref.merge_frame(zero, fields[1], np.zeros((2, 512), np.int64), counts, origins, 0.0, 'ios')[0].tolist() == [0, 512]
    # the record round trip
    r = ref.expected_record(*fields, counts, origins, 0.6, 'ios')
    u = ref.unpack_records(r)
    assert r.shape == (ref.REC_WORDS,) and int(u['count']) == 2 and u['index'][:3].tolist() == [0, 512, 0]
    assert u['bbox'][:2].tolist() == [[60, 50, 40, 20], [70, 50, 20, 20]] and u['class_idx'][:3].tolist() == [0, 3, 0]
    assert not u['pad'].any() and not u['bbox'][2:].any() and not u['score'][2:].any()


def _meta_detector():
    from mydetection_amd.api import Detector
    from mydetection_amd.models.general import name_to_model
    with torch.device('meta'):
        m, cfg = name_to_model('yolov3_80')
    return Detector(model_and_cfg=(m.eval(), cfg))


def test_tiles_value_class():
    from mydetection_amd.api import Tiles
    t = Tiles((640, 640))
    assert (t.size, t.overlap, t.full_frame, t.nms_thres, t.metric) == ((640, 640), 0.2, True, None, 'iou')
    assert Tiles(96).size == (96, 96) and Tiles((96, 128), 0.25, False, 0.6, 'ios').nms_thres == 0.6
    with pytest.raises(ValueError, match='metric'):
        Tiles((96, 128), metric='giou')
    with pytest.raises(ValueError, match='overlap'):
        Tiles((96, 128), overlap=1.0)
    with pytest.raises(ValueError, match='size'):
        Tiles((96, 0))


def test_detector_rejects_bad_tiled_calls_before_any_gpu_work():
    from mydetection_amd.api import Tiles
    det = _meta_detector()
    assert next(det.model.parameters()).device.type == 'meta'
    a, b = np.zeros((2, 150, 200, 3), np.uint8), np.zeros((1, 200, 150, 3), np.uint8)
    with pytest.raises(ValueError, match='one size'):
        det.predict_frames([a, b], tiles=Tiles((96, 128)))
    with pytest.raises(ValueError, match='one size'):
        det.frames_to_json([a, b], [0, 1, 2], tiles=Tiles((96, 128)))
    with pytest.raises(ValueError, match="'ios'"):
        det.predict_frames(a, tiles=Tiles((96, 128), metric='ios'), rotated_nms=True)
    for wrong in ((96, 128), 'tiles', True):
        with pytest.raises(TypeError, match='Tiles'):
            det.predict_frames(a, tiles=wrong)
    with pytest.raises(TypeError, match='float32'):                               # the frame rules hold as without tiles
        det.predict_frames(np.zeros((2, 8, 8, 3), np.float32), tiles=Tiles((96, 128)))
    with pytest.raises(ValueError, match='windows'):
        det.predict_frames(np.zeros((1, 1080, 1920, 3), np.uint8), tiles=Tiles((64, 64)))
    # 4:2:0: even frame and tile sizes, checked on the host
    y, uv = np.zeros((2, 96, 128), np.uint8), np.zeros((2, 48, 64, 2), np.uint8)
    with pytest.raises(ValueError, match='align'):
        det.predict_frames_yuv((y, uv), 'nv12', tiles=Tiles((63, 96)))
    with pytest.raises(ValueError, match='align'):
        det.predict_frames_nv12(np.zeros((2, 95, 127), np.uint8), np.zeros((2, 48, 64, 2), np.uint8), tiles=Tiles((64, 96)))
    with pytest.raises(ValueError, match="'ios'"):
        det.frames_nv12_to_json(y, uv, [0, 1], tiles=Tiles((64, 96), metric='ios'), rotated_nms=True)
    with pytest.raises(TypeError, match='Tiles'):
        det.frames_yuv_to_json((y, uv), 'nv12', [0, 1], tiles=(64, 96))
    # an empty batch (the last one of a video reader) is no error without tiles: nothing in, nothing out
    assert det.predict_frames([]) == [] and det.frames_to_json([], []) == []
    with pytest.raises(ValueError, match='one size'):
        det.predict_frames([], tiles=Tiles((96, 128)))
    # the argument rules come before any attribute of the detector is read
    from mydetection_amd.api import Detector
    with pytest.raises(TypeError, match='Tiles'):
        Detector.__new__(Detector).predict_frames(a, tiles='x')
    with pytest.raises(TypeError, match='tracker'):
        Detector.__new__(Detector).annotate_frames(np.zeros((8, 8, 3), np.float32), tracker='x')


def test_merge_tile_records_has_no_cpu_path():
    from mydetection_amd import _lib, ops
    rec = torch.zeros((3, _lib.REC_WORDS), dtype=torch.int32)
    with pytest.raises(RuntimeError):
        ops.merge_tile_records(rec, 1, 3, [(0, 0)] * 3, 0.5)
    with pytest.raises(ValueError, match='metric'):
        ops.merge_tile_records(rec, 1, 3, [(0, 0)] * 3, 0.5, metric='giou')
