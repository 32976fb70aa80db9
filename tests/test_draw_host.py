"""CPU-only: the host side of the overlay renderer -- the documented colour, text and palette rules, the numpy restatement
(tests/_draw_ref.py) anchored to PIL.ImageDraw, the argument rules of every layer, and the cap on unsettled pixels that
tests/test_gpu_draw.py relies on for rotated boxes."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import _draw_cases as cases
import _draw_ref as ref
from mydetection_amd import _lib, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIANTS = [('bt601', False), ('bt601', True), ('bt709', False), ('bt709', True)]
ISSUE_TABLE = {('bt601', False): ((66, 129, 25), (-38, -74, 112), (112, -94, -18)),
               ('bt601', True): ((77, 150, 29), (-43, -85, 128), (128, -107, -21)),
               ('bt709', False): ((47, 157, 16), (-26, -86, 112), (112, -102, -10)),
               ('bt709', True): ((54, 183, 18), (-29, -99, 128), (128, -116, -12))}


def test_rgb_to_yuv_table_and_header():
    for (matrix, full), rows in ISSUE_TABLE.items():
        got = ops.DRAW_YUV_ROWS[(ops.yuv_matrix_id(matrix), int(full))]
        assert got[:3] == rows and got[3] == (0 if full else 16)
    header = open(os.path.join(ROOT, 'include', 'mydet.h')).read()
    names = {0: 'BT.601', 1: 'BT.709'}
    for (m, full), (yr, ur, vr, _) in ops.DRAW_YUV_ROWS.items():
        pat = rf'\*\s+{m} \({re.escape(names[m])}\), {full}\s+' + r'\s+'.join(str(v) for v in yr + ur + vr) + r'\s*\n'
        assert re.search(pat, header), (m, full)
    # unit values: the defining identity on a few colours, written out
    c = np.array([[255, 0, 0], [12, 200, 99]], dtype=np.uint8)
    out = ops.rgb_to_yuv(c, 'bt601', False)
    assert out.tolist() == [[((66 * 255 + 128) >> 8) + 16, ((-38 * 255 + 128) >> 8) + 128, ((112 * 255 + 128) >> 8) + 128],
                            [((66 * 12 + 129 * 200 + 25 * 99 + 128) >> 8) + 16, ((-38 * 12 - 74 * 200 + 112 * 99 + 128) >> 8) + 128,
                             ((112 * 12 - 94 * 200 - 18 * 99 + 128) >> 8) + 128]]


@pytest.mark.parametrize('matrix,full', VARIANTS)
def test_rgb_to_yuv_within_one_of_float64_over_all_colours(matrix, full):
    kr, kb = (0.299, 0.114) if matrix == 'bt601' else (0.2126, 0.0722)
    kg = 1.0 - kr - kb
    ys, cs, yo = (1.0, 1.0, 0.0) if full else (219.0 / 255.0, 224.0 / 255.0, 16.0)
    g, b = np.meshgrid(np.arange(256), np.arange(256), indexing='ij')
    worst = 0
    for r in range(256):
        rgb = np.stack([np.full_like(g, r), g, b], axis=-1).reshape(-1, 3)
        got = ops.rgb_to_yuv(rgb.astype(np.uint8), matrix, full).astype(np.int64)
        R, G, B = (rgb[:, k].astype(np.float64) for k in range(3))
        y = kr * R + kg * G + kb * B
        want = np.stack([y * ys + yo, (B - y) / (2 * (1 - kb)) * cs + 128.0, (R - y) / (2 * (1 - kr)) * cs + 128.0], axis=-1)
        want = np.clip(np.rint(want), 0, 255).astype(np.int64)
        worst = max(worst, int(np.abs(got - want).max()))
    assert worst <= 1
    grey = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, axis=1)
    assert (ops.rgb_to_yuv(grey, matrix, full)[:, 1:] == 128).all()


def test_restatement_outline_equals_pil_rectangle():
    """Axis-aligned boxes with integer edges and even t: the restatement's outline is PIL's rectangle of width t."""
    from PIL import Image, ImageDraw
    H, W = 96, 160
    for x1, y1, x2, y2, t in ((20, 10, 70, 50, 2), (5, 5, 150, 90, 6), (30, 40, 34, 44, 2), (60, 20, 61, 80, 4), (-10, 30, 40, 120, 2),
                              (100, 60, 140, 64, 8)):
        row = np.array([(x1 + x2) / 2, (y1 + y2) / 2, x2 - x1, y2 - y1, 0.0])
        _, outline, unsettled = ref.box_masks(H, W, row, t, 0)
        img = Image.new('L', (W, H), 0)
        ImageDraw.Draw(img).rectangle([x1 - t // 2, y1 - t // 2, x2 + t // 2 - 1, y2 + t // 2 - 1], outline=255, width=t)
        assert np.array_equal(outline, np.asarray(img) != 0), (x1, y1, x2, y2, t)
        assert not unsettled.any()


def test_draw_label_text():
    assert ops.draw_label_text(3, 0.995, None) == '3 1.00'
    assert ops.draw_label_text(3, 0.994, 7) == '3 0.99 #7'
    assert ops.draw_label_text(0, float('nan'), None) == '0 0.00'
    assert ops.draw_label_text(0, -0.5, None) == '0 0.00' and ops.draw_label_text(0, float('inf'), None) == '0 1.00'
    assert ops.draw_label_text(0, 0.004999, None) == '0 0.00' and ops.draw_label_text(0, 0.005, None) == '0 0.01'
    names = ['person', 'a' * 20]
    assert ops.draw_label_text(1, 0.5, 10 ** 10 + 42, names) == 'a' * 16 + ' 0.50 #42'
    assert ops.draw_label_text(5, 0.5, -1, names) == '5 0.50 #9999999999'        # outside the table: the index; id mod 10^10
    assert ops.draw_label_text(0, 0.25, 9, names, ('score',)) == '0.25' and ops.draw_label_text(0, 0.25, 9, names, ('id', 'class')) == 'person #9'
    assert len(ops.draw_label_text(1, 1.0, 10 ** 10 - 1, names)) == _lib.DRAW_MAX_GLYPHS
    assert ops.draw_label_text(1, 0.5, 3, names, ()) == ''
    with pytest.raises(ValueError):
        ops.draw_label_text(0, 0.5, 1, None, ('klass',))


def test_glyph_atlas():
    for height in (8, 16, 24):
        a = ops.glyph_atlas(height)
        assert a.dtype == torch.uint8 and a.shape[0] == 96 and a.shape[1] == height and 1 <= a.shape[2] <= 64
        assert int(a.max()) == 1
        assert int(a[0].sum()) == 0                                   # the space
        assert all(int(a[c - 32].sum()) > 0 for c in range(33, 127))  # every printable glyph
        digits = [a[ord(d) - 32].numpy().tobytes() for d in '0123456789']
        assert len(set(digits)) == 10
    assert ops.glyph_atlas(16) is ops.glyph_atlas(16) or torch.equal(ops.glyph_atlas(16), ops.glyph_atlas(16))
    for bad in (7, 65):
        with pytest.raises(ValueError):
            ops.glyph_atlas(bad)


def test_draw_palette():
    p = ops.draw_palette(256)
    assert p.dtype == np.uint8 and p.shape == (256, 3) and np.array_equal(p, ops.draw_palette(256))
    assert np.array_equal(p[:16], ops.draw_palette(16))
    assert len({tuple(v) for v in p.tolist()}) == 256
    assert p[0].tolist() == [255, 0, 0] and p[1].tolist() == [0, 74, 255]
    h = 946 % 1530                                                   # entry 1 by hand: sector 3, f = 181 -> (0, 255 - 181, 255)
    assert (h // 255, h % 255) == (3, 181)
    with pytest.raises(ValueError):
        ops.draw_palette(0)


def test_draw_argument_rules_touch_no_device():
    from mydetection_amd.api import Detector, Draw
    for kw in (dict(thickness=0), dict(thickness=65), dict(thickness=2.5), dict(fill_alpha=256), dict(fill_alpha=-1), dict(color_by='hue'),
               dict(color=(1, 2)), dict(color=(1, 2, 300)), dict(labels=('name',)), dict(label_height=7), dict(label_height=65),
               dict(color_by='fixed'), dict(n_palette=0)):
        with pytest.raises(ValueError):
            ops.draw_style(**kw)
    with pytest.raises(TypeError):
        ops.draw_style(class_names=[1, 2])
    for kw in (dict(thickness=0), dict(labels=('x',)), dict(label_height=100), dict(fill_alpha=300), dict(color_by='fixed'), dict(color=(1, 2))):
        with pytest.raises(ValueError):
            Draw(**kw)
    assert Draw().style((1080, 1920)).thickness == 3 and Draw().style((1080, 1920)).label_height == 24
    assert Draw().style((96, 160)).thickness == 1 and Draw().style((96, 160), tracked=True).color_mode == _lib.DRAW_COLOR_ID
    assert Draw(color=(1, 2, 3)).style((96, 160)).color_mode == _lib.DRAW_COLOR_FIXED

    st = ops.draw_style()
    fr = torch.zeros((2, 8, 8, 3), dtype=torch.uint8)
    bx = torch.zeros((2, 3, 4))
    with pytest.raises(TypeError):
        ops.draw_boxes(fr.float(), bx, st)
    with pytest.raises(TypeError):
        ops.draw_boxes(fr, bx.double(), st)
    with pytest.raises(TypeError):
        ops.draw_boxes(fr, bx, 'style')
    with pytest.raises(TypeError):
        ops.draw_boxes(fr, bx, st, scores=torch.zeros((2, 3), dtype=torch.float64))
    with pytest.raises(TypeError):
        ops.draw_boxes(fr, bx, st, classes=torch.zeros((2, 3), dtype=torch.int32))
    with pytest.raises(TypeError):
        ops.draw_boxes(fr, bx, st, counts=torch.zeros(2, dtype=torch.int64))
    for bad in (dict(frames=fr[..., :2]), dict(frames=fr[:, :, :, [2, 1, 0]].permute(0, 2, 1, 3)), dict(boxes=torch.zeros((2, 3, 6))),
                dict(boxes=torch.zeros((3, 3, 4))), dict(scores=torch.zeros((2, 4))), dict(counts=torch.zeros(3, dtype=torch.int32)),
                dict(frames=fr[:, :, ::2])):
        args = dict(frames=fr, boxes=bx, style=st)
        args.update(bad)
        with pytest.raises(ValueError):
            ops.draw_boxes(**args)
    with pytest.raises(RuntimeError):                                 # everything is in order: only now the device matters
        if torch.cuda.is_available():
            raise RuntimeError('host tensors on a GPU machine are refused by require_gpu as well')
        ops.draw_boxes(fr, bx, st)

    y, uv = torch.zeros((2, 9, 9), dtype=torch.uint8), torch.zeros((2, 5, 5, 2), dtype=torch.uint8)
    for layout in ('p010', 'i010'):
        with pytest.raises(ValueError, match=layout):
            ops.draw_boxes_yuv420((y.short(), uv.short()), layout, bx, st)
    with pytest.raises(ValueError):
        ops.draw_boxes_yuv420((y, uv), 'nv16', bx, st)
    with pytest.raises(ValueError):
        ops.draw_boxes_yuv420((y, uv), 'nv12', bx, st, matrix='bt2020')
    with pytest.raises(ValueError):
        ops.draw_boxes_yuv420((y, uv[:, :4]), 'nv12', bx, st)
    with pytest.raises(ValueError):
        ops.draw_boxes_yuv420((y, uv), 'i420', bx, st)
    with pytest.raises(TypeError):
        ops.draw_boxes_yuv420((y.float(), uv), 'nv12', bx, st)
    with pytest.raises(ValueError):
        ops.draw_boxes_yuv420((y[:, :, ::2], uv[:, :, :3]), 'nv12', bx, st)

    records = torch.zeros((2, _lib.REC_WORDS), dtype=torch.int32)
    rec = ops.record_views(records)
    copies = {k: v.clone() for k, v in rec.items()}
    with pytest.raises(ValueError, match='copies'):
        ops.draw_records(fr, copies, st)
    with pytest.raises(TypeError):
        ops.draw_records(fr, records, st)
    with pytest.raises(ValueError):
        ops.draw_records(fr[:1], rec, st)
    with pytest.raises(ValueError, match='p010'):
        ops.draw_records((y.short(), uv.short()), rec, st, layout='p010')

    det = Detector.__new__(Detector)                                  # the argument rules come before the model is used
    with pytest.raises(TypeError):
        det.annotate_frames(np.zeros((8, 8, 3), np.uint8), draw='yes')
    with pytest.raises(TypeError):
        det.annotate_frames(np.zeros((8, 8, 3), np.float32))
    with pytest.raises(ValueError):
        det.annotate_frames([np.zeros((8, 8, 3), np.uint8), np.zeros((9, 8, 3), np.uint8)])
    with pytest.raises(TypeError):
        det.annotate_frames(np.zeros((8, 8, 3), np.uint8), tracker='t')
    with pytest.raises(ValueError, match='p010'):
        det.annotate_frames_yuv((np.zeros((8, 8), np.uint16), np.zeros((4, 4, 2), np.uint16)), 'p010')
    with pytest.raises(ValueError):
        det.annotate_frames_yuv((np.zeros((8, 8), np.uint8), np.zeros((4, 4, 2), np.uint8)), 'nv12', matrix='x')
    with pytest.raises(TypeError):
        det.annotate_frames_nv12(np.zeros((8, 8), np.uint8), np.zeros((4, 4, 2), np.uint8), draw=3)
    with pytest.raises(ValueError):
        det.annotate_frames_nv12(np.zeros((8, 8), np.uint8), np.zeros((4, 3, 2), np.uint8))
    with pytest.raises(NotImplementedError):
        det.detect_one(pil_img=__import__('PIL.Image').Image.new('RGB', (8, 8)), show_img=True)


def test_draw_entry_points_report_bad_arguments_before_launch():
    lib = _lib.lib()
    null = ctypes.c_void_p(0)
    one = ctypes.c_void_p(4096)                                       # a non-null address that is never dereferenced: every call fails its checks
    lst, st = _lib.DrawList(), _lib.DrawStyle()

    def rgb(dst=one, B=1, H=8, W=8, img=192, row=24, l=lst, s=st):
        return lib.mydet_draw_boxes_rgb_u8(dst, B, H, W, img, row, ctypes.byref(l) if l is not None else null,
                                           ctypes.byref(s) if s is not None else null, null)

    def good():
        l, s = _lib.DrawList(), _lib.DrawStyle()
        l.box, l.box_frame_stride, l.box_row_stride, l.K = 4096, 20, 4, 5
        s.thickness, s.color_mode = 2, _lib.DRAW_COLOR_FIXED
        return l, s
    assert rgb(l=None) == -1 and rgb(s=None) == -1
    l, s = good()
    assert rgb(dst=null, l=l, s=s) == -1 and rgb(B=0, l=l, s=s) == -1 and rgb(H=0, l=l, s=s) == -1 and rgb(W=-1, l=l, s=s) == -1
    assert rgb(row=23, l=l, s=s) == -1 and rgb(img=-1, l=l, s=s) == -1
    for field, value in (('box', None), ('K', 0), ('K', 513), ('box_row_stride', -1), ('score_frame_stride', -4), ('count_stride', -1)):
        l, s = good()
        setattr(l, field, value)
        assert rgb(l=l, s=s) == -1, field
    for field, value in (('thickness', 0), ('thickness', 65), ('fill_alpha', 256), ('fill_alpha', -1), ('color_mode', 3), ('color_mode', 0),
                         ('label_flags', 8), ('label_flags', 1), ('n_names', 0)):
        l, s = good()
        if field == 'n_names':
            s.names = 4096
        setattr(s, field, value)
        assert rgb(l=l, s=s) == -1, (field, value)
    for ch, cw in ((7, 8), (65, 8), (16, 0), (16, 65)):               # labels with an atlas of a cell size outside the range
        l, s = good()
        s.label_flags, s.atlas, s.ch, s.cw = 3, 4096, ch, cw
        assert rgb(l=l, s=s) == -1, (ch, cw)

    def yuv(layout=_lib.YUV420_NV12, matrix=0, full=0, planes=(4096, 8192, None), rows=(8, 8, 0), l=None, s=None, src=True):
        d = _lib.Yuv420Src()
        for i, p in enumerate(planes):
            d.plane[i], d.img_bytes[i], d.row_bytes[i] = p, 64, rows[i]
        d.layout, d.matrix, d.full_range = layout, matrix, full
        gl, gs = good()
        return lib.mydet_draw_boxes_yuv420_u8(ctypes.byref(d) if src else null, 1, 8, 8, ctypes.byref(l or gl), ctypes.byref(s or gs), null)
    assert yuv(src=False) == -1
    assert yuv(layout=_lib.YUV420_P010) == -1 and yuv(layout=_lib.YUV420_I010, planes=(4096, 8192, 12288), rows=(16, 8, 8)) == -1
    assert yuv(layout=7) == -1 and yuv(matrix=2) == -1 and yuv(full=2) == -1
    assert yuv(planes=(None, 8192, None)) == -1 and yuv(planes=(4096, None, None)) == -1
    assert yuv(planes=(4096, 8192, 12288)) == -1                      # a third plane for a semi-planar layout
    assert yuv(layout=_lib.YUV420_I420, planes=(4096, 8192, None), rows=(8, 4, 4)) == -1
    assert yuv(rows=(7, 8, 0)) == -1 and yuv(rows=(8, 7, 0)) == -1
    assert yuv(layout=_lib.YUV420_I420, planes=(4096, 8192, 12288), rows=(8, 4, 3)) == -1
    l, s = good()
    s.thickness = 0
    assert yuv(s=s) == -1

    # The same rows to the six entry points that take a list: draw, redact and crop, each rgb and yuv420.  A row changes one
    # thing of a call that is in order and names, per entry point, the code at B = 1 and at B = 65536 -- a batch every entry
    # point refuses with MYDET_E_UNSUPP (-2) once the checks before that one have passed, so -2 says "accepted so far" and
    # pins where each entry point puts that check.  None at B = 1: the call is in order and would launch; it is not sent.
    rst, out = _lib.RedactStyle(), _lib.CropOut()
    rst.mode, rst.shape, rst.cell, rst.pad = _lib.REDACT_MOSAIC, _lib.REDACT_BOX, 4, 1.0
    out.ch, out.cw, out.M, out.kind, out.pad, out.out, out.slot_stride, out.frame_stride = 8, 8, 1, _lib.CROP_U8, 1.0, 4096, 192, 192

    def six(B, l=True, row=24, layout=_lib.YUV420_NV12, planes=(4096, 8192, None), rows=(8, 8, 0), **fields):
        """The six calls, not yet made."""
        gl, gs = good()
        for k, v in fields.items():
            setattr(gl, k, v)
        lp = ctypes.byref(gl) if l else null
        d = _lib.Yuv420Src()
        for i, p in enumerate(planes):
            d.plane[i], d.img_bytes[i], d.row_bytes[i] = p, 64, rows[i]
        d.layout = layout
        return (lambda: lib.mydet_draw_boxes_rgb_u8(one, B, 8, 8, 192, row, lp, ctypes.byref(gs), null),
                lambda: lib.mydet_draw_boxes_yuv420_u8(ctypes.byref(d), B, 8, 8, lp, ctypes.byref(gs), null),
                lambda: lib.mydet_redact_boxes_rgb_u8(one, B, 8, 8, 192, row, lp, ctypes.byref(rst), one, null),
                lambda: lib.mydet_redact_boxes_yuv420_u8(ctypes.byref(d), B, 8, 8, lp, ctypes.byref(rst), one, null),
                lambda: lib.mydet_crop_boxes_rgb(one, B, 8, 8, 192, row, lp, ctypes.byref(out), null),
                lambda: lib.mydet_crop_boxes_yuv420(ctypes.byref(d), B, 8, 8, lp, ctypes.byref(out), null))

    N = None
    #      the row                                             draw rgb, yuv; redact rgb, yuv; crop rgb, yuv: at B = 1, at B = 65536
    table = ((dict(),                                          (N, N, N, N, N, N), (-2, -2, -2, -2, -2, -2)),
             (dict(l=False),                                   (-1,) * 6, (-1,) * 6),
             (dict(K=0),                                       (-1,) * 6, (-1,) * 6),
             (dict(K=513),                                     (-1,) * 6, (-1,) * 6),
             (dict(box_row_stride=-1),                         (-1,) * 6, (-1,) * 6),
             (dict(angle_frame_stride=-1),                     (-1,) * 6, (-1,) * 6),
             (dict(count_stride=-1),                           (-1,) * 6, (-1,) * 6),
             # planes that crop does not read: their strides are nothing to it
             (dict(score_row_stride=-1),                       (-1, -1, -1, -1, N, N), (-1, -1, -1, -1, -2, -2)),
             (dict(cls_frame_stride=-8),                       (-1, -1, -1, -1, N, N), (-1, -1, -1, -1, -2, -2)),
             (dict(id_row_stride=-1),                          (-1, -1, -1, -1, N, N), (-1, -1, -1, -1, -2, -2)),
             # a 10-bit layout: the painters refuse it, crops read it; redact checks the batch before the planes
             (dict(layout=_lib.YUV420_P010, rows=(16, 16, 0)), (N, -1, N, -1, N, N), (-2, -1, -2, -2, -2, -2)),
             (dict(planes=(4096, 8192, 12288)),                (N, -1, N, -1, N, -1), (-2, -1, -2, -2, -2, -1)),      # plane[2] for NV12
             (dict(row=23, rows=(7, 8, 0)),                    (-1,) * 6, (-1, -1, -2, -2, -2, -1)),                  # row_bytes one short
             (dict(row=24, rows=(8, 7, 0)),                    (N, -1, N, -1, N, -1), (-2, -1, -2, -2, -2, -1)))
    for row, small, large in table:
        assert tuple(call() for call in six(65536, **row)) == large, row
        assert tuple(N if want is N else call() for call, want in zip(six(1, **row), small)) == small, row


def test_unsettled_pixels_of_the_rotated_cases_stay_under_the_cap():
    """What tests/test_gpu_draw.py relies on: float32 error in (a, b) is below 1e-3 px for |coordinates| <= 512 (ulp 6e-5, a
    handful of roundings, sin / cos within a few ulp), so only pixels within 1e-3 of a deciding threshold may differ -- and in
    every rotated case those are at most 0.5 % of the painted pixels."""
    for name, H, W, t, alpha, frames in cases.rotated_cases():
        style = ops.draw_style(thickness=t, fill_alpha=alpha, color=(255, 255, 255))
        for boxes in frames:
            img = np.zeros((H, W, 3), dtype=np.uint8)
            unsettled = ref.draw_rgb(img, boxes, None, style)
            painted = int((img != 0).any(axis=2).sum())
            assert painted > 300, name
            print(name, int(unsettled.sum()), painted)
            assert unsettled.sum() <= 0.005 * painted, (name, int(unsettled.sum()), painted)
