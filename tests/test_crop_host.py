"""CPU-only: the host side of the object chips -- properties of the numpy restatement (tests/_crop_ref.py), the condition on the
cases of tests/_crop_cases.py that keeps the comparison of tests/test_gpu_crop.py from being hollow (every axis-aligned value
settled, at least 80 % of the rotated ones), the C ABI (declared, exported, bound, constants, the ABI version unchanged, argument
checks before any launch) and the argument rules of ops.crop_* and api.Chips."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import _crop_cases as cases
import _crop_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('mydet_crop_boxes_rgb', 'mydet_crop_boxes_yuv420')


def _img(H=40, W=56, seed=3):
    return np.random.default_rng(seed).integers(0, 256, size=(H, W, 3), dtype=np.uint8)


@pytest.mark.parametrize('chip', cases.CHIPS)
def test_a_box_on_the_pixel_grid_gives_the_pixels_and_quarter_turns_their_rotations(chip):
    ch, cw = chip
    img = _img()
    x0, y0 = 9, 5
    block = img[y0:y0 + ch, x0:x0 + cw]
    v, lo, hi = ref.chip(img, [x0 + cw / 2, y0 + ch / 2, cw, ch, 0], chip)
    assert np.array_equal(v, block) and np.array_equal(lo, v) and np.array_equal(hi, v)
    v, lo, hi = ref.chip(img, [x0 + cw / 2, y0 + ch / 2, cw, ch, 180], chip)
    assert np.array_equal(v, block[::-1, ::-1]) and np.array_equal(lo, hi)
    # a quarter turn: the box's w runs down the frame, so the source block is cw rows by ch columns ... of a box w = cw, h = ch
    # at 90 degrees the chip's x axis points down the frame and its y axis to the left
    tall = img[y0:y0 + cw, x0:x0 + ch]                                # cw rows, ch columns
    v, lo, hi = ref.chip(img, [x0 + ch / 2, y0 + cw / 2, cw, ch, 90], chip)
    assert np.array_equal(v, np.transpose(tall, (1, 0, 2))[::-1]) and np.array_equal(lo, hi)
    v, lo, hi = ref.chip(img, [x0 + ch / 2, y0 + cw / 2, cw, ch, 270], chip)
    assert np.array_equal(v, np.transpose(tall, (1, 0, 2))[:, ::-1]) and np.array_equal(lo, hi)
    for same, angle in ((0, 360), (90, -270), (270, -90), (180, -180), (90, 450)):
        assert np.array_equal(ref.chip(img, [20.5, 17.25, cw * 1.5, ch * 0.75, same], chip)[0],
                              ref.chip(img, [20.5, 17.25, cw * 1.5, ch * 0.75, angle], chip)[0])


def test_outside_the_frame_is_the_fill_colour_and_so_are_rows_that_are_no_boxes():
    img = _img()
    fill = (7, 201, 94)
    for row in ([-100, -100, 12, 24, 0], [500, 10, 12, 24, 33], [3e9, 10, 12, 24, 0], [10, 10, float('inf'), 5, 0], [10, 10, 0, 5, 0],
                [10, 10, 5, -1, 0], [float('nan'), 10, 5, 5, 0], [10, 10, 5, 5, float('nan')], [10, 10, 3e38, 3e38, 45]):
        v, lo, hi = ref.chip(img, row, (16, 8), 1.25, fill)
        assert (v == np.asarray(fill, np.uint8)).all() and np.array_equal(lo, v) and np.array_equal(hi, v), row
    # half outside: the outside half is fill, the inside half the pixels
    v, _, _ = ref.chip(img, [0, 8, 8, 16, 0], (16, 8), 1.0, fill)
    assert (v[:, :4] == np.asarray(fill, np.uint8)).all() and np.array_equal(v[:, 4:], img[0:16, 0:4])


def test_downscale_averages_and_the_sample_counts_follow_the_scale():
    img = _img()
    g = ref.geometry([20, 20, 8 * 0.75, 16 * 1.5, 0], (16, 8), 1.0)
    assert (g['nx'], g['ny']) == (1, 2)
    g = ref.geometry([20, 20, 8 * 5, 16 * 4.0, 0], (16, 8), 1.0)
    assert (g['nx'], g['ny']) == (4, 4)
    g = ref.geometry([20, 20, 8 * 2.5, 16 * 1.0, 0], (16, 8), 1.0)
    assert (g['nx'], g['ny']) == (3, 1)
    # an exact 2x downscale on the pixel grid: every chip pixel is the rounded mean of its 2 x 2 source pixels
    v, _, _ = ref.chip(img, [4 + 8, 6 + 16, 16, 32, 0], (16, 8))
    src = img[6:38, 4:20].astype(np.int64).reshape(16, 2, 8, 2, 3)
    assert np.array_equal(v, (src.sum(axis=(1, 3)) + 2) // 4)


def test_float_form_is_the_uint8_form_divided_and_normalised():
    v = np.arange(256, dtype=np.uint8).reshape(1, 16, 16)[..., None].repeat(3, axis=-1)
    f = ref.to_float(v, False)
    assert f.shape == (1, 3, 16, 16) and f.dtype == np.float32
    assert np.array_equal(f[0, 1].ravel(), np.arange(256, dtype=np.float32) / np.float32(255))
    n = ref.to_float(v, True)
    for c in range(3):
        want = (np.arange(256, dtype=np.float32) / np.float32(255) - np.float32(ref.IMAGENET_MEAN[c])) / np.float32(ref.IMAGENET_STD[c])
        assert np.array_equal(n[0, c].ravel(), want)
    from mydetection_amd import ops
    assert ops.IMAGENET_MEAN == ref.IMAGENET_MEAN and ops.IMAGENET_STD == ref.IMAGENET_STD


@pytest.mark.parametrize('case', cases.all_cases(), ids=lambda c: f'{c[0]}-{c[1]}-{c[2][0]}x{c[2][1]}-{c[3]}')
def test_cases_are_settled_enough_for_the_gpu_comparison(case):
    """Every axis-aligned and quarter-turn value is settled; in the rotated cases at least 80 % are, and the conditions under
    which the tolerance is derived hold for every rotated box."""
    kind, n, chip, pad = case
    H, W = cases.SIZES[n]
    value, lo, hi, written = cases.ref_chips(*case)
    boxes, counts = cases.case_boxes(kind, H, W, chip)
    assert written.sum() == counts.sum() and written[0].all()
    settled = (lo == hi)[written]
    assert ((lo <= value) & (value <= hi)).all()
    frac = settled.mean()
    print(case, 'settled', frac)
    if kind == 'axis':
        assert settled.all()
        skipped = value[0, -cases.SKIPPED_ROWS:]
        assert (skipped == np.asarray(cases.FILL, np.uint8)).all()
        assert (value[0, 8:10] == np.asarray(cases.FILL, np.uint8)).all()         # the two boxes wholly outside
        assert len({value[0, m].tobytes() for m in range(len(boxes[0]) - cases.SKIPPED_ROWS)}) >= 14
    else:
        assert frac >= 0.8
        assert all(ref.within_bound(row, chip, pad) for row in boxes[0])
        assert (value[written] != np.asarray(cases.FILL, np.uint8)).any(axis=-1).mean() > 0.6


def _header():
    return open(os.path.join(ROOT, 'include', 'mydet.h')).read()


def test_entry_points_are_declared_exported_and_bound():
    from mydetection_amd import _lib
    header = _header()
    dll = ctypes.CDLL(_lib.LIB_PATH)
    for name, nargs in zip(NAMES, (9, 7)):
        assert re.search(r'\bint\s+' + name + r'\s*\(', header)
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name]) == nargs
        assert hasattr(dll, name)
        assert getattr(_lib.lib(), name).argtypes == _lib.SIGNATURES[name]
    for name, value in (('MYDET_CROP_MAX_SIDE', 256), ('MYDET_CROP_MAX_SLOTS', 512), ('MYDET_CROP_U8', 0), ('MYDET_CROP_F32', 1)):
        assert re.search(r'#define\s+' + name + r'\s+' + str(value) + r'\b', header)
        assert getattr(_lib, name[len('MYDET_'):]) == value
    assert 'typedef struct mydet_crop_out' in header
    assert re.search(r'#define\s+MYDET_ABI_VERSION\s+2\b', header) and _lib.ABI_VERSION == 2 and _lib.lib().mydet_abi_version() == 2
    s = _lib.CropOut
    assert ctypes.sizeof(s) == 72 and s.pad.offset == 16 and s.fill.offset == 20 and s.mean3.offset == 32 and s.out.offset == 48
    assert s.slot_stride.offset == 56 and s.frame_stride.offset == 64
    # the rules the restatement is written from are in the header and in DESIGN.md
    design = open(os.path.join(ROOT, 'DESIGN.md')).read()
    for text in ('floorf((X - 0.5f) * 32 + 0.5f)', '+ 512) >> 10', 'clamp((int)ceilf(sx), 1, 4)'):
        assert text in header and text in design, text
    mk = open(os.path.join(ROOT, 'mydetection_amd', 'csrc', 'Makefile')).read()
    assert re.search(r'SRCS_EXACT\s*=.*\bcrop\.hip\b', mk)


def test_abi_argument_checks_come_before_any_launch():
    """Every call below must fail its checks: the pointers are never dereferenced on the device."""
    from mydetection_amd import _lib
    lib = _lib.lib()
    null = ctypes.c_void_p(0)
    mean = (ctypes.c_float * 3)(0.5, 0.5, 0.5)

    def good():
        l, o = _lib.DrawList(), _lib.CropOut()
        l.box, l.box_frame_stride, l.box_row_stride, l.K = 4096, 20, 4, 5
        o.ch, o.cw, o.M, o.kind, o.pad, o.out, o.slot_stride, o.frame_stride = 16, 8, 4, _lib.CROP_U8, 1.0, 8192, 384, 1536
        return l, o

    def rgb(src=ctypes.c_void_p(4096), B=1, H=8, W=8, img=192, row=24, l=None, o=None, no_list=False, no_out=False):
        gl, go = good()
        return lib.mydet_crop_boxes_rgb(src, B, H, W, img, row, null if no_list else ctypes.byref(l or gl), null if no_out else ctypes.byref(o or go),
                                        null)
    assert rgb(no_list=True) == -1 and rgb(no_out=True) == -1 and rgb(src=null) == -1
    assert rgb(B=0) == -1 and rgb(H=0) == -1 and rgb(W=-1) == -1 and rgb(row=23) == -1 and rgb(img=-1) == -1
    for field, value in (('box', None), ('K', 0), ('K', 513), ('box_row_stride', -1), ('box_frame_stride', -1), ('angle_row_stride', -4),
                         ('count_stride', -1)):
        l, o = good()
        setattr(l, field, value)
        assert rgb(l=l) == -1, field
    for field, value in (('ch', 0), ('ch', 257), ('cw', 0), ('cw', 257), ('M', 0), ('M', 513), ('kind', 2), ('kind', -1), ('pad', 0.0), ('pad', -1.0),
                         ('pad', float('nan')), ('pad', float('inf')), ('out', None), ('slot_stride', 383), ('slot_stride', -1),
                         ('frame_stride', -1), ('norm', 1)):
        l, o = good()
        setattr(o, field, value)
        assert rgb(o=o) == -1, (field, value)
    l, o = good()
    o.norm, o.mean3 = 1, ctypes.cast(mean, ctypes.c_void_p)          # std3 still null
    assert rgb(o=o) == -1

    def yuv(layout=_lib.YUV420_NV12, matrix=0, full=0, planes=(4096, 8192, None), rows=(8, 8, 0), o=None, src=True):
        d = _lib.Yuv420Src()
        for i, p in enumerate(planes):
            d.plane[i], d.img_bytes[i], d.row_bytes[i] = p, 64, rows[i]
        d.layout, d.matrix, d.full_range = layout, matrix, full
        gl, go = good()
        return lib.mydet_crop_boxes_yuv420(ctypes.byref(d) if src else null, 1, 8, 8, ctypes.byref(gl), ctypes.byref(o or go), null)
    assert yuv(src=False) == -1 and yuv(layout=7) == -1 and yuv(matrix=2) == -1 and yuv(full=2) == -1
    assert yuv(planes=(None, 8192, None)) == -1 and yuv(planes=(4096, None, None)) == -1 and yuv(planes=(4096, 8192, 12288)) == -1
    assert yuv(layout=_lib.YUV420_I420, planes=(4096, 8192, None), rows=(8, 4, 4)) == -1
    assert yuv(rows=(7, 8, 0)) == -1 and yuv(rows=(8, 7, 0)) == -1
    assert yuv(layout=_lib.YUV420_P010, rows=(15, 16, 0)) == -1 and yuv(layout=_lib.YUV420_P010, planes=(4097, 8192, None), rows=(16, 16, 0)) == -1
    l, o = good()
    o.cw = 0
    assert yuv(o=o) == -1


def test_chips_and_crop_argument_rules_touch_no_device():
    from mydetection_amd import _lib, ops
    from mydetection_amd.api import Chips, Detector
    c = Chips()
    assert c.size == (128, 64) and c.pad == 1.0 and c.max_per_frame == 64 and c.out == 'input' and c.fill == (0, 0, 0)
    assert Chips(size=[32, 16], out='uint8').kwargs('RGB_1_norm') == dict(size=(32, 16), max_per_frame=64, pad=1.0, fill=(0, 0, 0), out='uint8',
                                                                         input_format='RGB_1_norm')
    for kw in (dict(size=(0, 8)), dict(size=(8, 257)), dict(size=8), dict(size=(8, 8, 8)), dict(pad=0), dict(pad=-1), dict(pad=float('nan')),
               dict(pad=float('inf')), dict(pad=1e-60), dict(max_per_frame=0), dict(max_per_frame=513), dict(max_per_frame=2.5),
               dict(max_per_frame=None), dict(out='float'), dict(out=None), dict(fill=(1, 2)), dict(fill=(1, 2, 256)), dict(fill=3)):
        with pytest.raises(ValueError):
            Chips(**kw)

    fr = torch.zeros((2, 8, 8, 3), dtype=torch.uint8)
    bx = torch.zeros((2, 3, 4))
    with pytest.raises(TypeError):
        ops.crop_boxes(fr.float(), bx, (8, 8))
    with pytest.raises(TypeError):
        ops.crop_boxes(fr, bx.double(), (8, 8))
    with pytest.raises(TypeError):
        ops.crop_boxes(fr, bx, (8, 8), counts=torch.zeros(2, dtype=torch.int64))
    for bad in (dict(frames=fr[..., :2]), dict(boxes=torch.zeros((2, 3, 6))), dict(boxes=torch.zeros((3, 3, 4))),
                dict(counts=torch.zeros(3, dtype=torch.int32)), dict(size=(8, 300)), dict(pad=0.0), dict(out='input', input_format='BGR'),
                dict(max_per_frame=1000)):
        args = dict(frames=fr, boxes=bx, size=(8, 8))
        args.update(bad)
        with pytest.raises(ValueError):
            ops.crop_boxes(**args)
    with pytest.raises(RuntimeError):                                 # everything is in order: only now the device matters
        if torch.cuda.is_available():
            raise RuntimeError('host tensors on a GPU machine are refused by require_gpu as well')
        ops.crop_boxes(fr, bx, (8, 8))

    y, uv = torch.zeros((2, 9, 9), dtype=torch.uint8), torch.zeros((2, 5, 5, 2), dtype=torch.uint8)
    with pytest.raises(ValueError, match='nv16'):
        ops.crop_boxes_yuv420((y, uv), 'nv16', bx, (8, 8))
    with pytest.raises(ValueError, match='bt2020'):
        ops.crop_boxes_yuv420((y, uv), 'nv12', bx, (8, 8), matrix='bt2020')
    with pytest.raises(ValueError):
        ops.crop_boxes_yuv420((y, uv[:, :4]), 'nv12', bx, (8, 8))
    with pytest.raises(TypeError):
        ops.crop_boxes_yuv420((y.float(), uv), 'nv12', bx, (8, 8))
    with pytest.raises(TypeError):
        ops.crop_boxes_yuv420((y, uv), 'p010', bx, (8, 8))            # 8-bit planes for a 16-bit layout

    records = torch.zeros((2, _lib.REC_WORDS), dtype=torch.int32)
    rec = ops.record_views(records)
    with pytest.raises(ValueError, match='copies'):
        ops.crop_records(fr, {k: v.clone() for k, v in rec.items()}, (8, 8))
    with pytest.raises(TypeError):
        ops.crop_records(fr, records, (8, 8))

    det = Detector.__new__(Detector)                                  # the argument rules come before the model is used
    with pytest.raises(TypeError):
        det.crop_frames(np.zeros((8, 8, 3), np.uint8), chips='yes')
    with pytest.raises(TypeError):
        det.crop_frames(np.zeros((8, 8, 3), np.float32))
    with pytest.raises(ValueError):
        det.crop_frames([np.zeros((8, 8, 3), np.uint8), np.zeros((9, 8, 3), np.uint8)])
    with pytest.raises(TypeError):
        det.crop_frames(np.zeros((8, 8, 3), np.uint8), tracker='t')
    with pytest.raises(ValueError, match='nv16'):
        det.crop_frames_yuv((np.zeros((8, 8), np.uint8), np.zeros((4, 4, 2), np.uint8)), 'nv16')
    with pytest.raises(ValueError):
        det.crop_frames_yuv((np.zeros((8, 8), np.uint8), np.zeros((4, 4, 2), np.uint8)), 'nv12', matrix='x')
    with pytest.raises(TypeError):
        det.crop_frames_nv12(np.zeros((8, 8), np.uint8), np.zeros((4, 4, 2), np.uint8), chips=3)
    with pytest.raises(ValueError):
        det.crop_frames_nv12(np.zeros((8, 8), np.uint8), np.zeros((4, 3, 2), np.uint8))
