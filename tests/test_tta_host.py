"""CPU tests of test-time augmentation: the Augment value class and its view plan, the C ABI of the mirrored input launches and
of the fusion of view records (declared, exported, bound, constants, argument checks before any launch), the argument errors of
ops.fuse_view_records and Detector(..., augment=) on a meta-device model, and self-checks of the numpy restatement
tests/_tta_ref.py on the crafted cases of tests/_tta_cases.py."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import _tta_cases as cases
import _tta_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {'mydet_fuse_view_records_scratch_bytes': 4, 'mydet_fuse_view_records_f32': 15, 'mydet_frames_to_input_flip_f32': 24,
         'mydet_yuv420_to_input_flip_f32': 22}


def test_augment_views_and_argument_rules():
    from mydetection_amd.api import Augment
    a = Augment()
    assert a.views == ((1.0, 0), (1.0, 1)) and (a.fuse, a.metric, a.thres, a.min_score) == ('nms', 'iou', None, 0.0)
    for hflip in (False, True):
        for vflip in (False, True):
            got = Augment(hflip=hflip, vflip=vflip, scales=(1.0, 0.75)).views
            assert list(got) == ref.view_plan((1.0, 0.75), hflip, vflip) and len(got) == 2 * (1 + hflip + vflip + (hflip and vflip))
    assert Augment(hflip=True, vflip=True).views == ((1.0, 0), (1.0, 1), (1.0, 2), (1.0, 3))            # '', 'h', 'v', 'hv'
    yolov5 = Augment(views=((1.0, ''), (0.83, 'h'), (0.67, '')))
    assert yolov5.views == ((1.0, 0), (0.83, 1), (0.67, 0))
    assert yolov5.plan(640, 32, 'resize_pad_square') == [(640, 0), (544, 1), (416, 0)]
    assert [s for s, _ in yolov5.plan(640, 32, 'resize_pad_square')] == [ref.view_input_size(640, s, 32) for s in (1.0, 0.83, 0.67)]
    assert Augment(scales=(0.01,), hflip=False).plan(128, 32, 'resize_pad_divisible') == [(32, 0)]        # never below one cell
    assert Augment(scales=(1.0,)).plan(100, 32, 'resize_pad_square') == [(100, 0), (100, 1)]              # scale 1 is the call's own size
    assert Augment().plan(None, 32, 'pad_divisible') == [(None, 0), (None, 1)]
    with pytest.raises(ValueError, match='input_size'):
        Augment(scales=(1.0, 0.5)).plan(None, 32, 'pad_divisible')
    assert len(Augment(hflip=True, vflip=True, scales=(1.0, 0.5)).views) == 8
    with pytest.raises(ValueError, match='views'):
        Augment(hflip=True, vflip=True, scales=(1.0, 0.5, 0.25))                                         # 12 views
    with pytest.raises(ValueError, match='views'):
        Augment(views=())
    with pytest.raises(ValueError, match='twice'):
        Augment(views=((1.0, 'h'), (0.5, ''), (1.0, 'h')))
    with pytest.raises(ValueError, match='twice'):
        Augment(scales=(1.0, 1.0))
    for scale in (0.0, -1.0, float('nan'), float('inf')):
        with pytest.raises(ValueError, match='scale'):
            Augment(scales=(scale,))
    with pytest.raises(ValueError, match='flip'):
        Augment(views=((1.0, 'x'),))
    with pytest.raises(ValueError, match='flip'):
        Augment(views=((1.0, 4),))
    with pytest.raises(ValueError, match='view'):
        Augment(views=(1.0,))
    with pytest.raises(ValueError, match="'ios'"):
        Augment(fuse='wbf', metric='ios')
    with pytest.raises(ValueError, match='fuse'):
        Augment(fuse='mean')
    with pytest.raises(ValueError, match='metric'):
        Augment(metric='giou')
    with pytest.raises(ValueError, match='min_score'):
        Augment(fuse='wbf', min_score=-0.1)
    assert Augment(fuse='wbf', thres=0.6, min_score=0.1).thres == 0.6 and 'wbf' in repr(Augment(fuse='wbf'))


def test_entry_points_are_declared_exported_and_bound():
    from mydetection_amd import _lib, ops
    header = open(os.path.join(ROOT, 'include', 'mydet.h')).read()
    assert re.search(r'\bint64_t\s+mydet_fuse_view_records_scratch_bytes\s*\(', header)
    for name in ('mydet_fuse_view_records_f32', 'mydet_frames_to_input_flip_f32', 'mydet_yuv420_to_input_flip_f32'):
        assert re.search(r'\bint\s+' + name + r'\s*\(', header), name
    handle = ctypes.CDLL(_lib.LIB_PATH)
    lib = _lib.lib()
    for name, nargs in NAMES.items():
        assert hasattr(handle, name), name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name]) == nargs
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name]
        decl = re.search(r'\b' + name + r'\s*\(([^;]*)\)\s*;', header).group(1)
        assert len(decl.split(',')) == nargs, name                                 # the prototype has as many arguments
    assert lib.mydet_fuse_view_records_scratch_bytes.restype == ctypes.c_int64
    # the flip forms take the arguments of the old entry points plus `flip` before `stream`
    for new, old in (('mydet_frames_to_input_flip_f32', 'mydet_frames_to_input_f32'), ('mydet_yuv420_to_input_flip_f32', 'mydet_yuv420_to_input_f32')):
        assert _lib.SIGNATURES[new] == _lib.SIGNATURES[old][:-1] + [ctypes.c_int, ctypes.c_void_p]

    def define(name):
        return int(re.search(r'#define ' + name + r'\s+(-?\d+)', header).group(1))
    assert define('MYDET_VIEWS_MAX') == _lib.VIEWS_MAX == ops.VIEWS_MAX == ref.VIEWS_MAX == 8
    assert (define('MYDET_FUSE_NMS'), define('MYDET_FUSE_WBF')) == (_lib.FUSE_NMS, _lib.FUSE_WBF) == (0, 1)
    assert (define('MYDET_VIEW_HFLIP'), define('MYDET_VIEW_VFLIP')) == (_lib.VIEW_HFLIP, _lib.VIEW_VFLIP) == (ref.HFLIP, ref.VFLIP) == (1, 2)
    assert define('MYDET_ABI_VERSION') == _lib.ABI_VERSION == lib.mydet_abi_version() == 2      # symbols were added, nothing changed
    assert ctypes.sizeof(_lib.FuseMode) == 24 and [f[0] for f in _lib.FuseMode._fields_] == \
        ['kind', 'metric', 'rotated_nms', 'agnostic', 'min_score', 'reserved']
    assert re.search(r'typedef struct mydet_fuse_mode \{\s*int kind;[^}]*int metric;[^}]*int rotated_nms, agnostic;[^}]*float min_score;'
                     r'[^}]*int reserved;\s*\} mydet_fuse_mode;', header)
    assert [ops.view_flip_bits(f) for f in ('', 'h', 'v', 'hv', 0, 1, 2, 3)] == [0, 1, 2, 3, 0, 1, 2, 3]
    for wrong in ('vv', 4, -1, 1.0, True, None):
        with pytest.raises(ValueError, match='flip'):
            ops.view_flip_bits(wrong)


def test_fusion_abi_argument_checks():
    """Every call below must fail before any launch: the pointers are host addresses."""
    from mydetection_amd import _lib
    lib = _lib.lib()
    size = lib.mydet_fuse_view_records_scratch_bytes
    assert size(2, 3, 4, 0) == 2 * 3 * 512 * (16 + 8 + 4 + 8) == lib.mydet_merge_tile_records_scratch_bytes(2, 3, 4)
    assert size(2, 3, 5, 0) == 2 * 3 * 512 * (20 + 8 + 4 + 8) and size(2, 3, 4, 1) == 2 * 3 * 512 * (16 + 8 + 4)
    assert size(0, 3, 4, 0) == size(2, 0, 4, 0) == size(2, 9, 4, 0) == size(2, 3, 3, 0) == size(2, 3, 4, 2) == size(2, 3, 5, 1) == 0
    assert size(1, 8, 5, 0) > 0
    buf = (ctypes.c_int32 * 64)()
    p = (ctypes.cast(buf, ctypes.c_void_p).value + 15) // 16 * 16
    W4, W5 = _lib.REC_WORDS, _lib.REC_ROT_WORDS

    def call(rec=p, vs=None, fs=None, B=2, V=3, bw=4, flips=(0, 1, 2), hw=(300, 400), thres=0.5, kind=0, metric=0, rot=0, agn=0,
             min_score=0.0, mode=True, out=p, scratch=p, nbytes=None):
        words = W5 if bw == 5 else W4
        vs = B * words if vs is None else vs
        fs = words if fs is None else fs
        nbytes = (size(B, V, bw, kind) or 1 << 30) if nbytes is None else nbytes
        host = None if flips is None else (ctypes.c_int32 * max(len(flips), 1))(*flips)
        m = _lib.FuseMode(kind, metric, rot, agn, min_score, 0)
        return lib.mydet_fuse_view_records_f32(rec, vs, fs, B, V, bw, host, hw[0], hw[1], thres, ctypes.byref(m) if mode else None, out,
                                               scratch, nbytes, None)
    bad, unsupp = -1, -2
    assert call(V=0, flips=()) == bad and call(V=9, flips=(0,) * 9) == bad and call(B=0) == bad
    assert call(flips=(0, 1, 4)) == bad and call(flips=(0, -1, 2)) == bad and call(flips=None) == bad
    assert call(hw=(0, 400)) == bad and call(hw=(300, -1)) == bad
    assert call(kind=2) == bad and call(kind=-1) == bad and call(mode=False) == bad
    assert call(min_score=-0.5) == bad and call(min_score=float('nan')) == bad and call(kind=1, min_score=-1e-9) == bad
    assert call(bw=3) == bad and call(bw=6) == bad and call(metric=2) == bad and call(agn=2) == bad
    assert call(rot=1) == bad                                                    # the rotated test needs the angle plane
    assert call(rec=None) == bad and call(out=None) == bad and call(scratch=None) == bad
    assert call(rec=p + 4) == bad and call(out=p + 8) == bad and call(scratch=p + 8) == bad
    assert call(vs=2 * W4 + 2) == bad and call(fs=W4 + 1) == bad and call(vs=-2 * W4) == bad and call(fs=-W4) == bad
    assert call(nbytes=size(2, 3, 4, 0) - 1) == bad and call(kind=1, nbytes=size(2, 3, 4, 1) - 1) == bad and call(nbytes=0) == bad
    # the combinations that are not provided
    assert call(bw=5, metric=1, rot=1) == unsupp and call(bw=5, rot=1, agn=1) == unsupp
    assert call(kind=1, bw=5) == unsupp and call(kind=1, metric=1) == unsupp and call(kind=1, bw=5, rot=1) == unsupp


def test_ops_fuse_view_records_raises_before_any_device():
    from mydetection_amd import _lib, ops
    rec = torch.zeros((6, _lib.REC_WORDS), dtype=torch.int32)
    rot = torch.zeros((6, _lib.REC_ROT_WORDS), dtype=torch.int32)
    ok = dict(B=2, V=3, flips=[0, 1, 2], frame_hw=(300, 400), thres=0.5)

    def call(r=rec, **kw):
        return ops.fuse_view_records(r, **dict(ok, **kw))
    for kw, match in ((dict(kind='mean'), 'kind'), (dict(metric='giou'), 'metric'), (dict(V=9), 'V'), (dict(V=0), 'V'), (dict(B=0), 'B'),
                      (dict(flips=[0, 1]), '3 flips'), (dict(flips=[0, 1, 5]), 'flip'), (dict(flips=['h', 'x', '']), 'flip'),
                      (dict(frame_hw=(0, 4)), 'frame size'), (dict(min_score=-1), 'min_score'), (dict(min_score=float('nan')), 'min_score'),
                      (dict(rotated_nms=True), 'cxcywhd'), (dict(kind='wbf', metric='ios'), 'wbf'), (dict(B=3), 'shape')):
        with pytest.raises(ValueError, match=match):
            call(**kw)
    with pytest.raises(ValueError, match='wbf'):
        call(rot, kind='wbf')
    with pytest.raises(ValueError, match='wbf'):
        call(rot, kind='wbf', rotated_nms=True)
    with pytest.raises(ValueError, match='rotated_nms'):
        call(rot, metric='ios', rotated_nms=True)
    with pytest.raises(ValueError, match='rotated_nms'):
        call(rot, agnostic=True, rotated_nms=True)
    with pytest.raises(ValueError, match='int32'):
        call(rec.float())
    with pytest.raises(RuntimeError):                                            # and there is no CPU path
        call()
    with pytest.raises(RuntimeError):
        ops.frames_to_input(torch.zeros((1, 8, 8, 3), dtype=torch.uint8), (None, (0, 0), (8, 8), None), None, flip=1)
    with pytest.raises(ValueError, match='flip'):
        ops.frames_to_input(torch.zeros((1, 8, 8, 3), dtype=torch.uint8), (None, (0, 0), (8, 8), None), None, flip=4)
    with pytest.raises(ValueError, match='flip'):
        ops.yuv420_to_input((torch.zeros((1, 8, 8), dtype=torch.uint8), torch.zeros((1, 4, 4, 2), dtype=torch.uint8)), 'nv12',
                            (None, (0, 0), (8, 8), None), None, flip='x')


def _meta_detector(name='yolov3_80', **kw):
    from mydetection_amd.api import Detector
    from mydetection_amd.models.general import name_to_model
    with torch.device('meta'):
        m, cfg = name_to_model(name)
    return Detector(model_and_cfg=(m.eval(), cfg), **kw)


def test_detector_rejects_bad_augmented_calls_before_any_gpu_work():
    import PIL.Image
    from mydetection_amd.api import Augment, Tiles
    det = _meta_detector()
    assert next(det.model.parameters()).device.type == 'meta' and det.augment is None
    a = np.zeros((2, 150, 200, 3), np.uint8)
    y, uv = np.zeros((2, 96, 128), np.uint8), np.zeros((2, 48, 64, 2), np.uint8)
    for wrong in (True, 'h', (1.0, 'h')):
        with pytest.raises(TypeError, match='Augment'):
            det.predict_frames(a, augment=wrong)
    with pytest.raises(ValueError, match='tiled'):
        det.predict_frames(a, augment=Augment(), tiles=Tiles((96, 128)))
    with pytest.raises(ValueError, match='tiled'):
        det.frames_nv12_to_json(y, uv, [0, 1], augment=Augment(), tiles=Tiles((64, 96)))
    with pytest.raises(ValueError, match='tiled'):
        det.annotate_frames(a, augment=Augment(), tiles=Tiles((96, 128)))
    with pytest.raises(ValueError, match='tiled'):
        det.crop_frames_yuv((y, uv), 'nv12', augment=Augment(fuse='wbf'), tiles=Tiles((64, 96)))
    with pytest.raises(ValueError, match='input_size'):
        det.predict_frames(a, augment=Augment(scales=(1.0, 0.5)), preprocessing='pad_divisible')
    with pytest.raises(ValueError, match='cxcywhd'):                              # rotated_nms needs a rotated model, as without augment
        det.predict_frames(a, augment=Augment(), rotated_nms=True)
    pil = PIL.Image.fromarray(a[0])
    for call in (lambda **kw: det.predict_batch([pil], **kw), lambda **kw: det.detect_one(pil_img=pil, **kw)):
        with pytest.raises(TypeError, match='Augment'):
            call(augment='h')
        with pytest.raises(ValueError, match='input_size'):
            call(augment=Augment(scales=(0.5,)), preprocessing='pad_divisible')
    # a detector-wide default is checked when the detector is made, and applies to the calls that do not say otherwise
    with pytest.raises(TypeError, match='Augment'):
        _meta_detector(augment='h')
    with_default = _meta_detector(augment=Augment())
    with pytest.raises(ValueError, match='tiled'):
        with_default.predict_frames(a, tiles=Tiles((96, 128)))
    assert with_default.predict_frames([]) == [] and det.predict_frames([], augment=Augment()) == []
    # rotated boxes have no mean: WBF is for the 'cxcywh' models
    rapid = _meta_detector('rapid')
    with pytest.raises(ValueError, match='wbf'):
        rapid.predict_frames(a, augment=Augment(fuse='wbf'))
    with pytest.raises(ValueError, match='wbf'):
        _meta_detector('rapid', augment=Augment(fuse='wbf'))
    with pytest.raises(ValueError, match="'ios'"):
        rapid.predict_frames(a, augment=Augment(metric='ios'), rotated_nms=True)


# ---- the restatement itself ----

def _wbf(c, **kw):
    opts = {k: c[k] for k in ('agnostic', 'min_score') if k in c}
    return ref.wbf_frame(*cases.fields(c), **dict(opts, **kw))


def test_view_transform_and_flip_frame():
    frame = np.arange(2 * 3 * 4 * 3, dtype=np.uint8).reshape(2, 3, 4, 3)
    assert np.array_equal(ref.flip_frame(frame, 0), frame)
    assert np.array_equal(ref.flip_frame(frame, 1), frame[:, :, ::-1]) and np.array_equal(ref.flip_frame(frame, 2), frame[:, ::-1])
    assert np.array_equal(ref.flip_frame(frame, 3), frame[:, ::-1, ::-1])
    assert np.array_equal(ref.flip_frame(frame[..., 0], 1, rows_axis=-2), frame[:, :, ::-1, 0])
    b = np.zeros((4, 512, 5), np.float32)
    b[:, 0] = (30.25, 40.5, 10, 20, 15)
    t = ref.view_transform(b, [0, 1, 2, 3], (300, 400))
    assert t[:, 0].tolist() == [[30.25, 40.5, 10, 20, 15], [369.75, 40.5, 10, 20, -15], [30.25, 259.5, 10, 20, -15], [369.75, 259.5, 10, 20, 15]]
    assert t.dtype == np.float32 and np.array_equal(ref.view_transform(t, [0, 1, 2, 3], (300, 400)), b)     # exact here: an involution
    # the pixel under a box centre is the same pixel: column x of the mirrored frame is column W-1-x, and a centre at x + 0.5 maps to W - x - 0.5
    assert ref.view_transform(np.array([[[2.5, 1.5, 1, 1]]], np.float32), [3], (3, 4))[0, 0].tolist() == [1.5, 1.5, 1, 1]


def test_wbf_one_view_without_overlaps_comes_back_sorted_with_scores_over_v():
    grid = cases.grid_over_the_cap()
    for V in (1, 2, 4):
        b, s, c = cases._blank(V)
        b[V - 1, :100], s[V - 1, :100], c[V - 1, :100] = grid['boxes'][0, :100], grid['scores'][0, :100], grid['cats'][0, :100]
        counts = [0] * (V - 1) + [100]
        out = ref.wbf_frame(b, s, c, counts, [0] * V, (300, 400), 0.5)
        assert out['count'] == 100
        order = np.lexsort((-s[V - 1, :100], c[V - 1, :100]))                      # class ascending, score descending
        assert np.array_equal(out['index'], (V - 1) * 512 + order) and np.array_equal(out['cls'], c[V - 1, order])
        assert np.array_equal(out['score'], s[V - 1, order] / np.float32(V))       # exact: V is a power of two
        assert np.array_equal(out['bbox'], b[V - 1, order])                        # integer boxes: the mean of one is itself


@pytest.mark.parametrize('V', [2, 3, 8])
def test_wbf_identical_views_give_the_input_back(V):
    """V views that agree: every cluster has V members, the weighted mean of equal corners is that corner (the sums are exact:
    a float32 product in float64, added at most 8 times), and mean score * min(V, V) / V is the score."""
    rng = np.random.Generator(np.random.PCG64(5))
    n = 60
    grid = cases.grid_over_the_cap()
    b, s, c = cases._blank(V)
    b[:, :n], c[:, :n] = grid['boxes'][0, :n], grid['cats'][0, :n]
    s[:, :n] = rng.permutation(np.linspace(0.1, 0.9, n)).astype(np.float32)
    flips = [v % 4 for v in range(V)]
    stored = ref.view_transform(b, flips, (300, 400))                             # mirrored into each view: exact on integers
    stats = {}
    out = ref.wbf_frame(stored, s, c, [n] * V, flips, (300, 400), 0.5, stats=stats)
    assert out['count'] == n and stats == dict(clusters=n, dropped=0, joined=n * (V - 1), late=0)
    order = np.lexsort((-s[0, :n], c[0, :n]))
    assert np.array_equal(out['bbox'], b[0, order]) and np.array_equal(out['score'], s[0, order]) and np.array_equal(out['index'], order)


def test_wbf_a_permutation_of_the_views_changes_only_index():
    for seed, V in ((1, 3), (2, 8)):
        c = cases.random_clusters(seed, V)
        base = _wbf(c)
        assert 5 < base['count'] < sum(c['counts'])                               # views were fused, and not into one box
        perm = list(range(1, V)) + [0]                                        # a rotation: no view keeps its place
        other = _wbf(cases.permuted(c, perm))
        for name in ('count', 'bbox', 'score', 'cls'):
            assert np.array_equal(base[name], other[name]), name                  # scores are distinct: order P is the same
        back = np.asarray(perm)[other['index'] >> 9] * 512 + (other['index'] & 511)
        assert np.array_equal(back, base['index']) and not np.array_equal(other['index'], base['index'])


def test_wbf_crafted_cases():
    C = cases.crafted_wbf()
    out = _wbf(C['equal scores'])
    assert out['count'] == 2 and out['index'].tolist() == [0, 1] and out['cls'].tolist() == [0, 1]
    assert out['bbox'].tolist() == [[100, 100, 20, 20], [300, 200, 40, 30]] and out['score'].tolist() == [0.5, 0.25]
    out = _wbf(C['equidistant'])                                                  # founders at x = 130 (j = 0) and 110; the third joins j = 0
    assert out['count'] == 2 and out['index'].tolist() == [0, 1] and out['bbox'][1].tolist() == [110, 50, 10, 10]
    assert 120 < out['bbox'][0, 0] < 130 and out['bbox'][0, 2] > 10
    out = _wbf(C['equidistant, founders exchanged'])                              # now the founder at x = 110 is j = 0
    assert out['index'].tolist() == [1, 0] and out['bbox'][1].tolist() == [130, 50, 10, 10] and out['bbox'][0, 2] > 10
    stats = {}
    out = _wbf(C['chain'], stats=stats)
    assert out['count'] == 1 and stats['joined'] == 2 and out['index'].tolist() == [0]
    assert _wbf(dict(C['chain'], counts=[1, 0, 1]))['count'] == 2                 # without the middle box the third does not reach the founder
    out = _wbf(C['zero areas'])
    assert out['count'] == 4 and sorted(out['index'].tolist()) == [0, 1, 512, 513]
    out = _wbf(C['empty views'])
    assert out['count'] == 1 and out['index'].tolist() == [512] and out['score'][0] == np.float32(np.float64(np.float32(0.7)) * (1 / 3))
    assert _wbf(C['no candidates'])['count'] == 0
    out = _wbf(C['scores not above zero'])
    assert out['count'] == 2 and out['index'].tolist() == [2, 513]
    cut, kept = _wbf(C['min_score cuts singletons']), _wbf(C['min_score zero keeps them'])
    assert kept['count'] == 4 and cut['count'] == 3 and 512 * 2 + 1 in kept['index'] and 512 * 2 + 1 not in cut['index']
    assert (cut['score'] >= np.float32(0.2)).all() and (kept['score'] < np.float32(0.2)).sum() == 1
    aware, agn = _wbf(C['two classes, class-aware']), _wbf(C['two classes, agnostic'])
    assert aware['count'] == 4 and agn['count'] == 2 and agn['cls'].tolist() == [2, 3] and agn['index'].tolist() == [513, 0]
    # a bad-class view fails the frame; so does a live candidate whose class the keys cannot hold
    assert _wbf(dict(C['equal scores'], counts=[2, -1]))['count'] == -1
    bad = dict(C['equal scores'], cats=np.where(C['equal scores']['cats'] == 1, 4096, C['equal scores']['cats']))
    assert _wbf(bad)['count'] == -1
    r = ref.tref.unpack_records(ref.wbf_record(*cases.fields(C['equal scores'])))
    assert int(r['count']) == 2 and not r['bbox'][2:].any() and not r['score'][2:].any() and not r['pad'].any()


def test_wbf_over_the_cap():
    c = cases.grid_over_the_cap()
    stats = {}
    out = _wbf(c, stats=stats)
    assert stats['clusters'] == 512 and stats['dropped'] > 400 and stats['late'] >= 40 and out['count'] == 512
    # the founders are the 512 best candidates that did not join: every dropped one scores below every founder of a singleton
    assert out['score'].min() > 0 and len(set(out['index'].tolist())) == 512


def test_nms_fusion_restatement_on_crafted_pairs():
    A = (100, 100, 20, 20, 30)
    c = cases.case([[(A, 0.9, 0)], [((104, 100, 20, 20, 30), 0.8, 0)]], [0, 1], 0.4, width=5)
    assert c['boxes'][1, 0].tolist() == [296, 100, 20, 20, -30]
    u = ref.tref.unpack_records(ref.nms_record(*cases.fields(c)))
    assert int(u['count']) == 1 and u['index'][0] == 0 and u['bbox'][0].tolist() == [100, 100, 20, 20] and u['angle'][0] == 30
    u = ref.tref.unpack_records(ref.nms_record(*cases.fields(dict(c, thres=0.9))))
    assert int(u['count']) == 2 and u['bbox'][1].tolist() == [104, 100, 20, 20] and u['angle'][1] == 30 and u['index'][1] == 512
    two = cases.case([[(A[:4], 0.9, 0)], [((104, 100, 20, 20), 0.8, 1)]], [2, 3], 0.4)
    assert int(ref.tref.unpack_records(ref.nms_record(*cases.fields(two)))['count']) == 2
    u = ref.tref.unpack_records(ref.nms_agnostic_record(*cases.fields(two)))
    assert int(u['count']) == 1 and u['class_idx'][0] == 0
