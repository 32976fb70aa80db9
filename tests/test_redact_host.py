"""CPU tests of the redaction: the numpy restatement of its rules (tests/_redact_ref.py) against numbers derived by hand, the
argument rules of ops.redact_style and api.Redact, and the cap on unsettled pixels that keeps the GPU comparison of
tests/test_gpu_redact.py honest.  No device is touched."""
import numpy as np
import pytest
import torch

import _draw_cases as cases
import _redact_ref as ref
from mydetection_amd import ops
from mydetection_amd.api import Draw, Redact


def _full(H, W):
    """One row that covers the whole frame, values at multiples of 1/8."""
    return np.array([[W / 2, H / 2, 2.0 * W, 2.0 * H, 0]], dtype=np.float32)


def test_a_constant_frame_is_unchanged_by_mosaic_and_smooth():
    for H, W in ((8, 12), (37, 53)):
        for mode in ('mosaic', 'smooth'):
            for cell in (4, 6, 16):
                img = np.full((H, W, 3), (7, 130, 255), dtype=np.uint8)
                uns = ref.redact_rgb(img, _full(H, W), None, ops.redact_style(mode, cell))
                assert not uns.any() and (img == (7, 130, 255)).all()
                Y, U, V = np.full((H, W), 91, np.uint8), np.full(((H + 1) // 2, (W + 1) // 2), 3, np.uint8), np.full(((H + 1) // 2, (W + 1) // 2), 250, np.uint8)
                ref.redact_yuv(Y, U, V, _full(H, W), None, ops.redact_style(mode, cell))
                assert (Y == 91).all() and (U == 3).all() and (V == 250).all()


def test_smooth_of_a_linear_ramp_is_the_ramp():
    """The bilinear interpolation of the cell means of a linear ramp is the ramp, at every pixel at least c away from the border
    (further out the clamped cells flatten it).  On 2*j + 2*i the mean of a whole cell is the integer 2*(J*c + I*c) + 2*(c - 1),
    so nothing rounds and the input comes back.  On 2*j + i the mean is 2*J*c + I*c + 3*(c - 1)/2, a half (c is even), which
    round-half-up lifts by 1/2; the interpolation then lands on input + 1/2 exactly and the final round-half-up gives input + 1."""
    H, W = 48, 80
    i, j = np.mgrid[0:H, 0:W]
    for cell in (4, 8, 16):
        inner = (slice(cell, H - cell), slice(cell, W - cell))
        for ramp, lift in ((2 * j + 2 * i, 0), (2 * j + i, 1)):
            img = np.repeat(ramp[..., None], 3, axis=2).astype(np.uint8)
            ref.redact_rgb(img, _full(H, W), None, ops.redact_style('smooth', cell))
            assert np.array_equal(img[inner].astype(np.int64), np.repeat(ramp[..., None], 3, axis=2)[inner] + lift), (cell, lift)
    # the chroma planes of a 4:2:0 frame use c/2 on their own grid: the same statement there
    ramp = (2 * j + 2 * i)[:H // 2, :W // 2]
    Y, U, V = np.zeros((H, W), np.uint8), ramp.astype(np.uint8), (255 - ramp).astype(np.uint8)
    ref.redact_yuv(Y, U, V, _full(H, W), None, ops.redact_style('smooth', 8))
    assert np.array_equal(U[4:-4, 4:-4], ramp[4:-4, 4:-4]) and np.array_equal(V[4:-4, 4:-4], 255 - ramp[4:-4, 4:-4])
    assert not np.array_equal(U, ramp)                                       # the border cells are clamped


def test_a_worked_frame_at_cell_4():
    """frame[i, j] = 10*i + j on 8 x 12, cell 4: cells 2 x 3.  The mean of cell (I, J) before rounding is 10*(4I + 1.5) + 4J + 1.5:
        16.5 20.5 24.5        rounded half up:  17 21 25
        56.5 60.5 64.5                          57 61 65
    Mosaic, pixel (5, 6): cell (1, 1) = 61.
    Smooth, pixel (3, 5): u = 2*5 + 1 - 4 = 7, J0 = 0, fx = 7, Ja = 0, Jb = 1; v = 2*3 + 1 - 4 = 3, I0 = 0, fy = 3, Ia = 0, Ib = 1;
        top = 1*17 + 7*21 = 164, bottom = 1*57 + 7*61 = 484, value = (5*164 + 3*484 + 32) / 64 = 2304 / 64 = 36.
    Smooth, pixel (0, 0): u = v = -3, J0 = I0 = -1, fx = fy = 5, every tap clamps to cell (0, 0): (8*8*17 + 32) / 64 = 17 (17.5 floored).
    On 8 x 10 the last cell column is clipped to columns 8, 9: n = 8, S = 2*(0 + 10 + 20 + 30) + 4*(8 + 9) = 188,
        mean = (2*188 + 8) / 16 = 24; below it S = 2*(40 + 50 + 60 + 70) + 68 = 508, mean = (1016 + 8) / 16 = 64."""
    i, j = np.mgrid[0:8, 0:12]
    plane = 10 * i + j
    assert np.array_equal(ref.cell_means(plane, 4), [[17, 21, 25], [57, 61, 65]])
    assert ref.mosaic(plane, 4)[5, 6] == 61
    assert ref.smooth(plane, 4)[3, 5] == 36 and ref.smooth(plane, 4)[0, 0] == 17
    assert np.array_equal(ref.cell_means(plane[:, :10], 4), [[17, 21, 24], [57, 61, 64]])
    # through redact_rgb: a box over columns 4..7 of rows 4..7 only -- the other pixels keep their values
    img = np.repeat(plane[..., None], 3, axis=2).astype(np.uint8)
    uns = ref.redact_rgb(img, np.array([[6.0, 6.0, 4.0, 4.0, 0]], np.float32), None, ops.redact_style('mosaic', 4))
    want = plane.copy()
    want[4:8, 4:8] = 61
    assert not uns.any() and np.array_equal(img[..., 1], want)
    # pad scales the box: 4 x 4 at pad 1.5 covers 6 x 6 pixel centres
    img = np.zeros((8, 12, 3), np.uint8)
    ref.redact_rgb(img, np.array([[6.0, 4.0, 4.0, 4.0, 0]], np.float32), None, ops.redact_style('solid', 4, pad=1.5, color=(1, 2, 3)))
    assert (img[1:7, 3:9] == (1, 2, 3)).all() and int((img[..., 0] == 1).sum()) == 36
    # the ellipse: centre (6, 4), ra = 3, rb = 2 -- pixel centre (6.5, 4.5) is in, (8.5, 5.5) is out ((2.5*2)^2 + (1.5*3)^2 = 45.25 > 36)
    img = np.zeros((8, 12, 3), np.uint8)
    ref.redact_rgb(img, np.array([[6.0, 4.0, 6.0, 4.0, 0]], np.float32), None, ops.redact_style('solid', 4, shape='ellipse', color=(9, 9, 9)))
    assert img[4, 6, 0] == 9 and img[5, 8, 0] == 0 and img[4, 8, 0] == 9          # (8.5, 4.5): (2.5*2)^2 + (0.5*3)^2 = 27.25 <= 36


def test_the_chroma_quad_rule_at_an_odd_frame_edge():
    """7 x 9 luma, 4 x 5 chroma.  A box over the last luma column and row alone (pixel (6, 8)) redacts chroma sample (3, 4), whose
    quad has that single pixel; a box over pixel (2, 3) alone redacts chroma (1, 1) and no other."""
    for rows, sample in (([[8.5, 6.5, 1.0, 1.0, 0]], (3, 4)), ([[3.5, 2.5, 1.0, 1.0, 0]], (1, 1))):
        Y, U, V = np.full((7, 9), 200, np.uint8), np.full((4, 5), 100, np.uint8), np.full((4, 5), 50, np.uint8)
        ref.redact_yuv(Y, U, V, np.array(rows, np.float32), None, ops.redact_style('solid', 4, color=(0, 0, 0)), 'bt601', True)
        y, u, v = ops.rgb_to_yuv(np.zeros(3, np.uint8), 'bt601', True)
        assert int((Y != 200).sum()) == 1 and Y[int(rows[0][1]), int(rows[0][0])] == y
        want_u, want_v = np.full((4, 5), 100, np.uint8), np.full((4, 5), 50, np.uint8)
        want_u[sample], want_v[sample] = u, v
        assert np.array_equal(U, want_u) and np.array_equal(V, want_v)
    # chroma cells are c/2 samples on the chroma grid: cell 6 on 7 x 9 gives chroma cells of 3 x 3 samples, the last ones clipped
    U = np.arange(20, dtype=np.int64).reshape(4, 5)
    assert np.array_equal(ref.cell_means(U, 3), [[6, 9], [16, 19]])         # 6, 8.5 -> 9, 16, 18.5 -> 19


def test_row_order_and_duplicated_rows_do_not_matter():
    H, W = cases.SIZES[1]
    rng = np.random.default_rng(3)
    rows = cases.random_boxes(77, H, W, 8, True)
    base = rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
    for mode in ('mosaic', 'smooth', 'solid'):
        st = ops.redact_style(mode, 6, shape='ellipse', pad=1.25)
        outs = []
        for order in (rows, rows[::-1], np.concatenate([rows, rows[2:5], rows[::-1]])):
            img = base.copy()
            ref.redact_rgb(img, order, None, st)
            outs.append(img)
        assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], outs[2]) and not np.array_equal(outs[0], base)
    # skipped rows, counts and the class filter
    st = ops.redact_style('solid', 4, classes=[2, 5], color=(1, 1, 1))
    img = base.copy()
    ref.redact_rgb(img, rows, 6, st, classes=np.array([2, 0, 5, 1, 1, 1, 2, 2]))
    want = base.copy()
    ref.redact_rgb(want, rows[[0, 2]], None, ops.redact_style('solid', 4, color=(1, 1, 1)))
    assert np.array_equal(img, want)
    for count in (0, -3):
        img = base.copy()
        ref.redact_rgb(img, rows, count, st, classes=np.full(8, 2))
        assert np.array_equal(img, base)


def test_redact_style_and_redact_value_errors():
    ok = ops.redact_style()
    assert (ok.mode, ok.cell, ok.shape, ok.pad, ok.classes, ok.color) == ('mosaic', 16, 'box', 1.0, None, (0, 0, 0))
    assert 'mosaic' in repr(ok) and 'Redact(' in repr(Redact()) and 'cell=None' in repr(Redact())
    bad = (dict(mode='blur'), dict(mode=None), dict(shape='circle'), dict(shape=1), dict(cell=5), dict(cell=2), dict(cell=66), dict(cell=8.0),
           dict(cell=True), dict(cell='8'), dict(pad=0), dict(pad=-1.0), dict(pad=float('nan')), dict(pad=float('inf')), dict(pad=1e-50),
           dict(pad='wide'), dict(classes=[]), dict(classes=list(range(17))), dict(classes=[1.5]), dict(classes=3), dict(classes=[2 ** 31]),
           dict(classes=['person']), dict(color=(1, 2)), dict(color=(0, 0, 256)), dict(color=(-1, 0, 0)), dict(color=None), dict(color='red'))
    for kw in bad:
        with pytest.raises(ValueError):
            ops.redact_style(**kw)
        with pytest.raises(ValueError):
            Redact(**kw)
    st = ops.redact_style('smooth', 64, 'ellipse', 1.25, classes=(0, 7), color=(1, 2, 3)).struct()
    assert (st.mode, st.shape, st.cell, st.pad, st.n_classes, list(st.classes[:2]), list(st.color[:3])) == (1, 1, 64, 1.25, 2, [0, 7], [1, 2, 3])
    assert Redact(cell=None).cell is None and Redact(cell=8).style((1080, 1920)).cell == 8


def test_the_default_cell_follows_the_frame_size():
    assert Redact.default_cell((96, 160)) == 4                              # 2 * ((96 + 48) // 96) = 2 -> the floor of 4
    assert Redact.default_cell((1080, 1920)) == 22 and Redact.default_cell((1920, 1080)) == 22
    assert Redact.default_cell((2160, 3840)) == 46
    assert Redact.default_cell((8000, 8000)) == 64
    r = Redact('smooth', pad=1.25)
    assert r.style((1080, 1920)).cell == 22 and r.style((2160, 3840)).cell == 46 and r.style((1080, 1920)) is r.style((1080, 1000000))
    assert r.style((96, 160)).mode == 'smooth' and r.style((96, 160)).pad == 1.25


def test_redact_arguments_of_the_wrong_type_and_ten_bit_layouts():
    from mydetection_amd.api import Detector
    for given in (Draw(), 'mosaic', ops.redact_style()):
        with pytest.raises(TypeError, match='Redact'):
            Detector._setting(given, Redact, 'redact_frames')
        with pytest.raises(TypeError, match='Redact'):
            Detector._redact_setting(given, 'annotate_frames')
    assert Detector._redact_setting(None, 'annotate_frames') is None and isinstance(Detector._setting(None, Redact, 'redact_frames'), Redact)
    frames = torch.zeros((1, 8, 8, 3), dtype=torch.uint8)
    with pytest.raises(TypeError, match='RedactStyle'):
        ops.redact_boxes(frames, torch.zeros((1, 1, 4)), Redact())
    with pytest.raises(TypeError, match='RedactStyle'):
        ops.redact_boxes(frames, torch.zeros((1, 1, 4)), ops.draw_style())
    planes = (torch.zeros((1, 8, 8), dtype=torch.int16), torch.zeros((1, 4, 4, 2), dtype=torch.int16))
    for layout in ('p010', 'i010'):
        with pytest.raises(ValueError, match=layout):
            ops.redact_boxes_yuv420(planes if layout == 'p010' else (planes[0], planes[1][..., 0], planes[1][..., 1]), layout,
                                    torch.zeros((1, 1, 4)), ops.redact_style())
    with pytest.raises(ValueError, match='class filter'):
        ops.redact_boxes(frames, torch.zeros((1, 1, 4)), ops.redact_style(classes=[1]))
    with pytest.raises(ValueError, match='512'):
        ops.redact_boxes(frames, torch.zeros((1, 513, 4)), ops.redact_style(), classes=torch.zeros((1, 513), dtype=torch.int64))


def _unsettled_share(H, W, rows, st):
    covered, uns = ref.coverage(H, W, rows, None, st)
    return int(uns.sum()), int(covered.sum())


def test_unsettled_pixels_stay_below_the_cap_of_the_gpu_comparison():
    """The GPU test compares rotated rows and ellipses on settled pixels only; that says something as long as the unsettled ones are
    few: at most 0.5 % of each frame's covered pixels, the renderer's cap, for the very lists the GPU test uses."""
    worst = 0.0
    for _, H, W, _, _, frames in cases.rotated_cases():
        for rows in frames:
            for pad in (1.0, 1.25):
                for shape in ('box', 'ellipse'):
                    n, covered = _unsettled_share(H, W, rows, ops.redact_style('mosaic', 4, shape, pad))
                    assert covered > 500 and n <= 0.005 * covered, (H, W, pad, shape, n, covered)
                    worst = max(worst, n / covered)
    print(f'rotated cases: worst unsettled share {100 * worst:.3f} %')
    for H, W in cases.SIZES:
        for pad in (1.0, 1.25):
            n, covered = _unsettled_share(H, W, cases.axis_boxes(H, W), ops.redact_style('mosaic', 4, 'ellipse', pad))
            print(f'axis_boxes ellipse {H}x{W} pad {pad}: {n} of {covered}')
            assert covered > 1000 and n <= 0.005 * covered, (H, W, pad, n, covered)
            # an axis-aligned box at multiples of 1/8 is exact in float32: nothing is unsettled, the GPU test compares with == everywhere
            n, covered = _unsettled_share(H, W, cases.axis_boxes(H, W), ops.redact_style('mosaic', 4, 'box', pad))
            assert n == 0 and covered > 1000
