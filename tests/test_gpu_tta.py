"""GPU tests of test-time augmentation, bit for bit throughout.

  * The mirrored input launches (mydet_frames_to_input_flip_f32, mydet_yuv420_to_input_flip_f32) against the unmirrored entry
    points on a mirrored copy, at the smallest shapes that reach every path of the tile pipeline.
  * The fusion of view records (mydet_fuse_view_records_f32): the NMS kind against the restatement of the merge of tile records on
    the transformed boxes (tests/_tta_ref.py; its pair values are float64, so the random inputs come from seeds for which no
    pair value of the selected candidates is within MARGIN of the threshold) and against ops.merge_tile_records itself; the
    WBF kind against tests/_tta_ref.py, whose float32 / float64 operations are the kernel's in the kernel's order.
  * Detector(..., augment=) against the same fusion applied to the detections of the mirrored frames through the public path.
"""
import ctypes
import types

import numpy as np
import PIL.Image
import pytest
import torch

import _tta_cases as cases
import _tta_ref as ref
import _yuv420_ref as yref
from _arena import flat_arena
from test_gpu_crop import _same_objects
from test_gpu_draw import _drawn_from_objects
from test_gpu_tiles import _assert_objects_equal_records, _records_of_objects, _synthetic_frames, detector  # noqa: F401

pytestmark = pytest.mark.gpu

tref = ref.tref
MARGIN = 1e-5
FORMATS = ('RGB_1', 'RGB_1_norm')
FLIP_DIMS = {1: [2], 2: [1], 3: [1, 2]}


def _geometry(h, w, name, size=None, div=32):
    from mydetection_amd.api import Detector
    return Detector._geometry(types.SimpleNamespace(divisibe=div), h, w, name, size)


def _frames(b, h, w, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    return torch.from_numpy(rng.integers(0, 256, size=(b, h, w, 3), dtype=np.uint8))


# (frame h, w), geometry.  Odd sizes; 37 x 150 under pad_divisible gives a 64 x 160 input: three x-tiles of 64, the last partial.
INPUT_CASES = {
    'pad_only_37x150': ((37, 150), lambda: _geometry(37, 150, 'pad_divisible')),                     # null tables
    'up_37x150_to_192': ((37, 150), lambda: _geometry(37, 150, 'resize_pad_divisible', 192)),        # upscale: two taps, clamped windows
    'down_75x301_to_150': ((75, 301), lambda: _geometry(75, 301, 'resize_pad_divisible', 150)),      # downscale: 7 taps, three x-tiles
    'steep_200x121_to_96': ((200, 121), lambda: _geometry(200, 121, 'resize_pad_divisible', 96)),    # several source-row steps per tile
    'square_37x150_to_160': ((37, 150), lambda: _geometry(37, 150, 'resize_pad_square', 160)),       # top != 0
    'square_53x37_to_64': ((53, 37), lambda: _geometry(53, 37, 'resize_pad_square', 64)),            # left != 0
    'odd_Wp_67': ((90, 71), lambda: ((44, 61), (3, 2), (50, 67), None)),                             # Wp % 4 != 0: the one-pixel store form
    'x_only_40x91_to_40x64': ((40, 91), lambda: ((40, 64), (0, 0), (64, 64), None)),                 # horizontal pass alone
    'y_only_91x40_to_64x40': ((91, 40), lambda: ((64, 40), (0, 8), (64, 64), None)),                 # vertical pass alone
}


@pytest.mark.parametrize('case', list(INPUT_CASES))
def test_mirrored_rgb_input_equals_the_input_of_the_mirrored_frames(case):
    from mydetection_amd import ops
    (h, w), geo = INPUT_CASES[case]
    geo = geo()
    if case == 'pad_only_37x150':
        assert geo[0] is None and geo[2] == (64, 160)
    if case == 'down_75x301_to_150':
        assert geo[0] == (37, 150) and geo[2] == (64, 160)
    if case.startswith('square'):
        assert max(geo[1]) > 0
    frames = _frames(2, h, w, seed=len(case)).cuda()
    for fmt in FORMATS:
        plain = ops.frames_to_input(frames, geo, fmt)
        assert torch.equal(ops.frames_to_input(frames, geo, fmt, flip=0), plain)
        for flip in (1, 2, 3):
            want = ops.frames_to_input(torch.flip(frames, FLIP_DIMS[flip]), geo, fmt)
            got = ops.frames_to_input(frames, geo, fmt, flip=flip)
            assert torch.equal(got, want), (case, fmt, flip, int((got != want).sum()))
            assert not torch.equal(got, plain)
        assert torch.equal(ops.frames_to_input(frames, geo, fmt, flip='hv'), want)


def test_mirrored_rgb_input_of_strided_frames_and_unaligned_outputs():
    """A crop view of a larger buffer is read in place (row and frame strides larger than the picture), and an `out` view that is
    not 16-byte aligned takes the one-pixel store form."""
    from mydetection_amd import ops
    h, w = 37, 150
    big = _frames(3, h + 9, w + 11, seed=7).cuda()
    view = big[:, 4:4 + h, 6:6 + w]
    assert not view.is_contiguous()
    for name, size in (('pad_divisible', None), ('resize_pad_square', 160), ('resize_pad_divisible', 96)):
        geo = _geometry(h, w, name, size)
        Hp, Wp = geo[2]
        for flip in (1, 2, 3):
            want = ops.frames_to_input(torch.flip(view, FLIP_DIMS[flip]).contiguous(), geo, 'RGB_1_norm')
            assert torch.equal(ops.frames_to_input(view, geo, 'RGB_1_norm', flip=flip), want), (name, flip)
            flat = torch.full((3 * 3 * Hp * Wp + 1,), 7.0, device='cuda')
            out = flat[1:].view(3, 3, Hp, Wp)
            assert out.data_ptr() % 16 == 4
            assert ops.frames_to_input(view, geo, 'RGB_1_norm', out=out, flip=flip) is out
            assert torch.equal(out, want) and float(flat[0]) == 7.0, (name, flip)
    assert torch.equal(big[:, 4:4 + h, 6:6 + w], view)


def test_mirrored_rgb_input_past_the_tap_limit_mirrors_a_copy():
    from mydetection_amd import _lib, ops
    frames = _frames(1, 600, 40, seed=3).cuda()
    geo = ((64, 40), (0, 0), (64, 64), None)                                     # 9.4x down: 21 taps
    from mydetection_amd.utils.image_ops import resample_tables
    assert resample_tables(600, 64)[1].shape[1] > _lib.FRAMES_MAX_TAPS
    for flip in (1, 2, 3):
        assert torch.equal(ops.frames_to_input(frames, geo, 'RGB_1', flip=flip), ops.frames_to_input(torch.flip(frames, FLIP_DIMS[flip]), geo, 'RGB_1'))


def _dev(a):
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).cuda()


def _offset(t):
    """The plane in an allocation of its own at an odd element offset with a wider pitch: the reads by samples of the 8-bit
    layouts (for 16-bit words: an address that is no multiple of 4)."""
    inner = int(np.prod(t.shape[2:]))
    buf = torch.zeros((t.shape[0], t.shape[1] + 1, inner + 7), dtype=t.dtype, device=t.device)
    view = buf[:, :t.shape[1], 1:1 + inner]
    view.copy_(t.reshape(t.shape[0], t.shape[1], inner))
    return view.unflatten(2, tuple(t.shape[2:])) if t.dim() == 4 else view


# odd sizes (a partial last quad and an odd chroma row), three x-tiles, an upscale, a downscale, top / left != 0
YUV_CASES = {
    'pad_only_37x150': ((37, 150), lambda: _geometry(37, 150, 'pad_divisible')),
    'pad_only_37x149': ((37, 149), lambda: _geometry(37, 149, 'pad_divisible')),
    'up_37x149_to_192': ((37, 149), lambda: _geometry(37, 149, 'resize_pad_divisible', 192)),
    'down_75x301_to_150': ((75, 301), lambda: _geometry(75, 301, 'resize_pad_divisible', 150)),
    'square_37x150_to_160': ((37, 150), lambda: _geometry(37, 150, 'resize_pad_square', 160)),
    'odd_Wp_67': ((90, 71), lambda: ((44, 61), (3, 2), (50, 67), None)),
    'even_96x128_to_64': ((96, 128), lambda: _geometry(96, 128, 'resize_pad_square', 64)),
}


@pytest.mark.parametrize('layout', yref.LAYOUTS)
@pytest.mark.parametrize('case', list(YUV_CASES))
def test_mirrored_yuv_input_equals_the_input_of_the_mirrored_rgb_frames(case, layout):
    """The mirrored source is the mirrored RGB image of the conversion (tests/_yuv420_ref.py), whatever the layout and for odd
    sizes too; where the frame is even, it is also the unmirrored call on the mirrored planes; and it is ops.frames_to_input on
    the mirrored ops.yuv420_to_rgb."""
    from mydetection_amd import ops
    (h, w), geo = YUV_CASES[case]
    geo = geo()
    planes = yref.random_planes(layout, 2, h, w, seed=len(case) + len(layout))
    rgb = yref.to_rgb(planes, layout, 'bt709', True)
    tight = tuple(_dev(p) for p in planes)
    kw = dict(matrix='bt709', full_range=True)
    fmt = 'RGB_1_norm'
    plain = ops.yuv420_to_input(tight, layout, geo, fmt, **kw)
    assert torch.equal(ops.yuv420_to_input(tight, layout, geo, fmt, flip=0, **kw), plain)
    assert torch.equal(plain, ops.frames_to_input(torch.from_numpy(rgb).cuda(), geo, fmt))
    on_device = ops.yuv420_to_rgb(tight, layout, **kw)
    for flip in (1, 2, 3):
        want = ops.frames_to_input(torch.from_numpy(ref.flip_frame(rgb, flip)).cuda(), geo, fmt)
        got = ops.yuv420_to_input(tight, layout, geo, fmt, flip=flip, **kw)
        assert torch.equal(got, want), (case, layout, flip, int((got != want).sum()))
        assert torch.equal(got, ops.frames_to_input(torch.flip(on_device, FLIP_DIMS[flip]), geo, fmt))
        shifted = tuple(_offset(t) for t in tight)
        assert torch.equal(ops.yuv420_to_input(shifted, layout, geo, fmt, flip=flip, **kw), want), (case, layout, flip, 'reads by samples')
        if h % 2 == 0 and w % 2 == 0:
            mirrored = tuple(_dev(ref.flip_frame(p, flip, rows_axis=1)) for p in planes)
            assert torch.equal(ops.yuv420_to_input(mirrored, layout, geo, fmt, flip=0, **kw), want)


# ---- the fusion of view records ----

def _records(c_list):
    """Cases of one V (one per frame) -> the [V,B,words] record buffer as numpy."""
    V = len(c_list[0]['flips'])
    return np.stack([np.stack([tref.pack_record(c['boxes'][v], c['scores'][v], c['cats'][v], c['counts'][v]) for c in c_list]) for v in range(V)])


def _fuse(rec, flips, frame_hw, thres, layout='view_major', **kw):
    """ops.fuse_view_records on a numpy [V,B,words] buffer -> the fused [B,words] buffer as numpy."""
    from mydetection_amd import ops
    V, B, words = rec.shape
    if layout == 'view_major':
        dev = torch.from_numpy(np.ascontiguousarray(rec)).cuda().view(V * B, words)
    else:                                                            # [B][V] in memory, handed over through its strides
        dev = torch.from_numpy(np.ascontiguousarray(rec.transpose(1, 0, 2))).cuda().transpose(0, 1)
        assert V == 1 or (dev.stride(0) == words and dev.stride(1) == V * words)
    out = ops.fuse_view_records(dev, B, V, flips, frame_hw, thres, **kw)
    torch.cuda.synchronize()
    assert out['records'].shape == (B, words) and out['index'].data_ptr() == out['records'].data_ptr() + 4 * tref.REC_INDEX
    return out['records'].cpu().numpy()


def _same_words(got, want, what):
    g, w = tref.unpack_records(got), tref.unpack_records(want)
    assert int(g['count']) == int(w['count']), (what, int(g['count']), int(w['count']))
    for name in w:
        bits = np.uint32 if w[name].dtype == np.float32 else w[name].dtype
        np.testing.assert_array_equal(g[name].view(bits), w[name].view(bits), err_msg=f'{what}: field {name}')
    np.testing.assert_array_equal(got, want)


def _merge_of_transformed(c_list, thres, **kw):
    """ops.merge_tile_records at zero origins on records whose boxes were brought back from their views on the host."""
    from mydetection_amd import ops
    V = len(c_list[0]['flips'])
    moved = [dict(c, boxes=ref.view_transform(c['boxes'], c['flips'], c['frame_hw'])) for c in c_list]
    rec = torch.from_numpy(_records(moved)).cuda()
    out = ops.merge_tile_records(rec.view(V * len(c_list), -1), len(c_list), V, [(0, 0)] * V, thres, **kw)
    torch.cuda.synchronize()
    return out['records'].cpu().numpy()


# seeds found on the CPU (tests/_tta_ref.nms_margin): no pair value of the selected candidates within MARGIN of the threshold
NMS_SEEDS = {('iou', 4, False): 1, ('ios', 4, False): 1, ('iou', 5, False): 1, ('iou', 5, True): 1}
NMS_COUNTS = [[60, 0, 45], [512, 300, 512]]                          # frame 1: 1 324 candidates, the top-k cut runs


def _nms_cases(metric, width, rotated_nms):
    seed = NMS_SEEDS[(metric, width, rotated_nms)]
    flips = [0, 1, 2] if width == 4 else [3, 1, 2]
    return [cases.random_clusters(seed + 100 * b, 3, width, n_obj=40, counts=n, thres=0.45, jitter=4.0, flips=flips) for b, n in enumerate(NMS_COUNTS)]


@pytest.mark.parametrize('layout', ['view_major', 'frame_major'])
@pytest.mark.parametrize('metric,width,rotated_nms', list(NMS_SEEDS))
def test_nms_fusion_against_the_restatement(metric, width, rotated_nms, layout):
    cs = _nms_cases(metric, width, rotated_nms)
    flips, hw, thres = cs[0]['flips'], cs[0]['frame_hw'], cs[0]['thres']
    rec = _records(cs)
    got = _fuse(rec, flips, hw, thres, layout, metric=metric, rotated_nms=rotated_nms)
    for b, c in enumerate(cs):
        m = ref.nms_margin(*cases.fields(c), metric, rotated_nms)
        assert m > MARGIN, f'frame {b} has a pair within {m:.2e} of the threshold; pick another seed'
        _same_words(got[b], ref.nms_record(*cases.fields(c), metric, rotated_nms), f'{metric} width {width} rot {rotated_nms} frame {b}')
    counts = tref.unpack_records(got)['count']
    assert 5 < counts[0] < 105 and 20 < counts[1] < 512              # boxes were suppressed, not everything
    views = {int(i) >> 9 for i in tref.unpack_records(got[1])['index'][:counts[1]]}
    assert views == {0, 1, 2}
    if width == 5:                                                   # the angle came back from its view: negated under one flip
        g = tref.unpack_records(got[1])
        idx = g['index'][:counts[1]]
        stored = cs[1]['boxes'][idx >> 9, idx & 511, 4]
        sign = np.where(np.isin(np.asarray(flips)[idx >> 9], (1, 2)), -1, 1).astype(np.float32)
        np.testing.assert_array_equal(g['angle'][:counts[1]], sign * stored)
    # and it is the merge of tile records on the transformed boxes, word for word
    np.testing.assert_array_equal(got, _merge_of_transformed(cs, thres, metric=metric, rotated_nms=rotated_nms))


@pytest.mark.parametrize('metric', ['iou', 'ios'])
@pytest.mark.parametrize('width', [4, 5])
def test_nms_fusion_agnostic(metric, width):
    cs = _nms_cases('iou', width, False)
    flips, hw, thres = cs[0]['flips'], cs[0]['frame_hw'], cs[0]['thres']
    got = _fuse(_records(cs), flips, hw, thres, metric=metric, agnostic=True)
    np.testing.assert_array_equal(got, _merge_of_transformed(cs, thres, metric=metric, agnostic=True))
    aware = _fuse(_records(cs), flips, hw, thres, metric=metric)
    n_agn, n_aware = tref.unpack_records(got)['count'], tref.unpack_records(aware)['count']
    assert (n_agn <= n_aware).all() and n_agn[1] < n_aware[1]        # boxes of different classes were joined
    if metric == 'iou':                                              # float32 pair values in the kernel's order: no margin to keep
        for b, c in enumerate(cs):
            _same_words(got[b], ref.nms_agnostic_record(*cases.fields(c)), f'agnostic width {width} frame {b}')


@pytest.mark.parametrize('width', [4, 5])
def test_nms_fusion_without_flips_is_the_merge_at_zero_origins(width):
    from mydetection_amd import ops
    cs = _nms_cases('iou', width, False)
    rec = torch.from_numpy(_records(cs)).cuda()
    V, B, words = rec.shape
    for kw in (dict(), dict(metric='ios'), dict(agnostic=True)) + ((dict(rotated_nms=True),) if width == 5 else ()):
        got = ops.fuse_view_records(rec.view(V * B, words), B, V, [0] * V, (300, 400), 0.45, **kw)
        want = ops.merge_tile_records(rec.view(V * B, words), B, V, [(0, 0)] * V, 0.45, **kw)
        assert torch.equal(got['records'], want['records']), kw


def test_nms_fusion_bad_class_view_and_unsupported_combinations():
    from mydetection_amd import _lib, ops
    C = cases.crafted_wbf()['equal scores']
    for counts in ([2, -1], [-1, 1], [-1, -1]):
        c = dict(C, counts=counts)
        for kind in ('nms', 'wbf'):
            got = _fuse(_records([c]), c['flips'], c['frame_hw'], 0.5, kind=kind)
            assert int(got[0, 0]) == -1 and not got[0, 1:].any(), (counts, kind)
    _same_words(_fuse(_records([C]), C['flips'], C['frame_hw'], 0.5)[0], ref.nms_record(*cases.fields(C)), 'crafted pair')
    lib = _lib.lib()
    for words, bw in ((_lib.REC_WORDS, 4), (_lib.REC_ROT_WORDS, 5)):
        rec = torch.zeros((2, words), dtype=torch.int32, device='cuda')
        out = torch.full((1, words), 7, dtype=torch.int32, device='cuda')
        nbytes = lib.mydet_fuse_view_records_scratch_bytes(1, 2, bw, 0)
        scratch = torch.empty(nbytes // 8, dtype=torch.int64, device='cuda')
        flips = (ctypes.c_int32 * 2)(0, 1)

        def call(kind, metric, rot, agn):
            mode = _lib.FuseMode(kind, metric, rot, agn, 0.0, 0)
            return lib.mydet_fuse_view_records_f32(ops._ptr(rec), words, words, 1, 2, bw, flips, 300, 400, 0.5, ctypes.byref(mode), ops._ptr(out),
                                                   ops._ptr(scratch), nbytes, ops._stream())
        if bw == 5:
            assert call(0, 1, 1, 0) == -2 and call(0, 0, 1, 1) == -2 and call(1, 0, 0, 0) == -2 and call(1, 0, 1, 0) == -2
        else:
            assert call(1, 1, 0, 0) == -2
        torch.cuda.synchronize()
        assert bool((out == 7).all())                                # nothing was launched
        assert call(0, 0, 1 if bw == 5 else 0, 0) == 0 and call(0, 1, 0, 1) == 0
        torch.cuda.synchronize()
        assert not out.any()                                         # no candidates: a record of zeros


def _wbf_check(c_list, layout='view_major', what=''):
    c0 = c_list[0]
    opts = {k: c0[k] for k in ('agnostic', 'min_score') if k in c0}
    got = _fuse(_records(c_list), c0['flips'], c0['frame_hw'], c0['thres'], layout, kind='wbf', **opts)
    outs = []
    for b, c in enumerate(c_list):
        stats = {}
        _same_words(got[b], ref.wbf_record(*cases.fields(c), stats=stats, **opts), f'wbf {what} frame {b}')
        outs.append((tref.unpack_records(got[b]), stats))
    return outs


@pytest.mark.parametrize('layout', ['view_major', 'frame_major'])
@pytest.mark.parametrize('V', [1, 2, 3, 8])
def test_wbf_random_clusters(V, layout):
    """Two frames of jittered views of shared objects; frame 1 has views of 512 boxes, so its chain is V*512 candidates long."""
    cs = [cases.random_clusters(10 + V, V)]
    cs.append(cases.random_clusters(20 + V, V, n_obj=120, counts=[512] * V, jitter=3.0, flips=cs[0]['flips']))
    (g0, s0), (g1, s1) = _wbf_check(cs, layout, f'V = {V}')
    assert s0['clusters'] >= 20 and s1['clusters'] >= 100 and s0['dropped'] == s1['dropped'] == 0
    if V > 1:
        assert s0['joined'] > 10 and s1['joined'] > 300                                          # views were fused
        assert (g0['score'][:int(g0['count'])] < 1).all() and len({int(i) >> 9 for i in g1['index'][:int(g1['count'])]}) > 1


@pytest.mark.parametrize('name', list(cases.crafted_wbf()))
def test_wbf_crafted(name):
    _wbf_check([cases.crafted_wbf()[name]], what=name)


def test_wbf_over_the_cluster_cap():
    (g, stats), = _wbf_check([cases.grid_over_the_cap()], what='cap')
    assert int(g['count']) == 512 and stats['clusters'] == 512 and stats['dropped'] > 400 and stats['late'] >= 40


def test_wbf_thresholds_and_agnostic_on_random_views():
    for kw in (dict(thres=0.3), dict(thres=0.8), dict(agnostic=True), dict(min_score=0.3), dict(thres=0.0), dict(thres=-1.0)):
        cs = [dict(cases.random_clusters(31, 3, flips=[2, 0, 1]), **kw), dict(cases.random_clusters(32, 3, flips=[2, 0, 1]), **kw)]
        _wbf_check(cs, what=str(kw))


@pytest.mark.parametrize('kind,width', [('nms', 4), ('nms', 5), ('wbf', 4)])
def test_fusion_footprint(kind, width):
    """records and scratch lie between sentinel guard bands: the bands are untouched, every word of the B records is written,
    and a scratch one byte short is refused."""
    from mydetection_amd import _lib, ops
    lib = _lib.lib()
    B, V = 2, 3
    cs = [cases.random_clusters(41, V, width, counts=[512, 30, 0], flips=[1, 2, 3]), cases.random_clusters(42, V, width, counts=[0, 0, 0], flips=[1, 2, 3])]
    rec = _records(cs)
    words = rec.shape[2]
    dev = torch.device('cuda')
    src = torch.from_numpy(rec).to(dev)
    k = _lib.FUSE_WBF if kind == 'wbf' else _lib.FUSE_NMS
    nbytes = lib.mydet_fuse_view_records_scratch_bytes(B, V, width, k)
    assert nbytes == B * V * 512 * (4 * width + (12 if kind == 'wbf' else 20))
    out, chk_out = flat_arena(B * words, dev)
    scratch, chk_scratch = flat_arena(nbytes // 4, dev)
    flips = (ctypes.c_int32 * V)(*cs[0]['flips'])
    mode = _lib.FuseMode(k, _lib.MERGE_IOU, 0, 0, 0.0, 0)

    def call(n):
        return lib.mydet_fuse_view_records_f32(ops._ptr(src), B * words, words, B, V, width, flips, 300, 400, 0.55, ctypes.byref(mode),
                                               ops._ptr(out), ops._ptr(scratch), n, ops._stream())
    assert call(nbytes - 1) == -1
    torch.cuda.synchronize()
    assert chk_out.undefined_in_view()[0] == B * words               # nothing was launched
    assert call(nbytes) == 0
    torch.cuda.synchronize()
    chk_out.outside_untouched('records')
    chk_scratch.outside_untouched('scratch')
    assert chk_out.undefined_in_view() == (0, [])
    got = out.view(torch.int32).view(B, words).cpu().numpy()
    want = ref.wbf_record(*cases.fields(cs[0])) if kind == 'wbf' else _merge_of_transformed(cs, 0.55)[0]
    np.testing.assert_array_equal(got[0], want)
    assert int(got[0, 0]) > 10 and not got[1].any()                  # a frame without detections: a record of zeros
    assert torch.equal(src.cpu(), torch.from_numpy(rec))             # the view records are only read


# ---- model level ----

H, W, B = 150, 200, 2
KW = dict(input_size=128, conf_thres=0.001)


def _view_records(det, frames, flips, sizes=None, **kw):
    """The [V,B,words] record buffer (device, view-major) of the mirrored frames through the public path.  Views of one input
    size go through ONE predict_frames call on the list of their mirrored copies, so that they make the batch the augmented
    call makes."""
    sizes = sizes or [KW['input_size']] * len(flips)
    out = [None] * len(flips)
    for size in dict.fromkeys(sizes):
        vs = [v for v, s in enumerate(sizes) if s == size]
        mirrored = torch.cat([torch.flip(frames, FLIP_DIMS[flips[v]]) if flips[v] else frames for v in vs])
        objs = det.predict_frames(mirrored, **dict(KW, input_size=size), **kw)
        rec = _records_of_objects(objs, len(vs), frames.shape[0])
        for n, v in enumerate(vs):
            out[v] = rec[n]
    return torch.from_numpy(np.stack(out)).cuda()


def _expected(det, frames, flips, sizes=None, thres=None, fuse_kw=None, **kw):
    from mydetection_amd import ops
    rec = _view_records(det, frames, flips, sizes, **kw)
    V, n = rec.shape[:2]
    return ops.fuse_view_records(rec.view(V * n, -1), n, V, flips, (H, W), det.nms_thres if thres is None else thres, **(fuse_kw or {}))


def _differs(objs, others):
    return any(len(a) != len(b) or not torch.equal(a.bboxes, b.bboxes) or not torch.equal(a.scores, b.scores) for a, b in zip(objs, others))


def test_augmented_predict_frames_equals_the_fusion_of_the_mirrored_calls(detector, monkeypatch):
    from mydetection_amd import ops
    from mydetection_amd.api import Augment
    name, det = detector
    frames = torch.from_numpy(_synthetic_frames(B, H, W, seed=70)).cuda()
    aug = Augment(hflip=True)
    calls = []
    real = ops.fuse_view_records
    monkeypatch.setattr(ops, 'fuse_view_records', lambda *a, **k: (calls.append((a, k)), real(*a, **k))[1])
    got = det.predict_frames(frames, augment=aug, **KW)
    assert len(calls) == 1 and calls[0][0][1:4] == (B, 2, [0, 1]) and calls[0][0][4:6] == ((H, W), det.nms_thres)
    want = _expected(det, frames, [0, 1])
    assert sum(want['count'].tolist()) > 0
    _assert_objects_equal_records(got, want, (H, W))
    plain = det.predict_frames(frames, **KW)
    assert _differs(got, plain), 'the fusion returned view 0: the test would show nothing'
    assert len({int(i) >> 9 for b, k in enumerate(want['count'].tolist()) for i in want['index'][b, :k].tolist()}) == 2
    # the records behind the objects
    (idxs, rec), = det._frame_records(frames, augment=aug, **KW)
    assert idxs == [0, 1] and rec['img_hw'] == [(H, W)] * B and torch.equal(rec['records'], want['records'])
    # by now the batch of 2B inputs has been seen more than twice: a captured graph is replayed, and gives the same bits
    assert any(k[0][0] == 2 * B for k in det._graphs.graphs)
    again = det.predict_frames(frames.cpu().numpy(), augment=aug, **KW)            # host frames this time
    _assert_objects_equal_records(again, want, (H, W))
    # augment=None is the call without the keyword
    none = det.predict_frames(frames, augment=None, **KW)
    assert not _differs(none, plain) and all(torch.equal(a.cats, b.cats) for a, b in zip(none, plain))
    # json rows
    eval_type = 'cxcywhd' if name == 'rapid' else 'x1y1wh'
    rows = det.frames_to_json(frames, [7, 8], eval_type, augment=aug, **KW)
    assert rows == [r for o, i in zip(got, (7, 8)) for r in o.to_json(i, eval_type)] and len(rows) > 0
    # a threshold and a metric of the fusion's own
    calls.clear()
    got = det.predict_frames(frames, augment=Augment(thres=0.3, metric='ios'), **KW)
    assert calls[0][0][5:8] == (0.3, 'nms', 'ios')
    _assert_objects_equal_records(got, _expected(det, frames, [0, 1], thres=0.3, fuse_kw=dict(metric='ios')), (H, W))
    # a detector-wide default
    det.augment = aug
    try:
        _assert_objects_equal_records(det.predict_frames(frames, **KW), want, (H, W))
        assert not _differs(det.predict_frames(frames, augment=None, **KW), plain)
    finally:
        del det.augment


def test_augmented_scales_run_two_input_sizes(detector):
    from mydetection_amd.api import Augment
    name, det = detector
    frames = torch.from_numpy(_synthetic_frames(B, H, W, seed=70)).cuda()
    aug = Augment(scales=(1.0, 0.75))
    assert aug.plan(128, det.divisibe, det.preprocess) == [(128, 0), (128, 1), (96, 0), (96, 1)]
    got = det.predict_frames(frames, augment=aug, **KW)
    want = _expected(det, frames, [0, 1, 0, 1], [128, 128, 96, 96])
    _assert_objects_equal_records(got, want, (H, W))
    views = {int(i) >> 9 for b, k in enumerate(want['count'].tolist()) for i in want['index'][b, :k].tolist()}
    assert views & {2, 3} and views & {0, 1}                         # both input sizes contribute
    # views given one by one, in an order that interleaves the two sizes
    mixed = Augment(views=((0.75, 'h'), (1.0, ''), (0.75, 'v')))
    got = det.predict_frames(frames, augment=mixed, **KW)
    _assert_objects_equal_records(got, _expected(det, frames, [1, 0, 2], [96, 128, 96]), (H, W))


def test_a_vertical_flip_negates_the_angles(detector):
    from mydetection_amd.api import Augment
    name, det = detector
    frames = torch.from_numpy(_synthetic_frames(B, H, W, seed=70)).cuda()
    got = det.predict_frames(frames, augment=Augment(views=((1.0, 'v'),)), **KW)
    flipped = det.predict_frames(frames.flip(1), **KW)
    assert sum(len(o) for o in got) > 0
    for g, f in zip(got, flipped):
        assert len(g) == len(f) and torch.equal(g.scores, f.scores) and torch.equal(g.cats, f.cats)
        assert torch.equal(g.bboxes[:, 0], f.bboxes[:, 0] + 0.0) and torch.equal(g.bboxes[:, 1], (float(H) - f.bboxes[:, 1]) + 0.0)
        assert torch.equal(g.bboxes[:, 2:4], f.bboxes[:, 2:4])
        if name == 'rapid':
            assert g.bboxes.shape[1] == 5 and torch.equal(g.bboxes[:, 4], -f.bboxes[:, 4]) and bool((g.bboxes[:, 4] != 0).any())
    both = det.predict_frames(frames, augment=Augment(views=((1.0, 'hv'),)), **KW)
    if name == 'rapid':                                              # two flips: a rotation by 180 degrees keeps the angle
        turned = det.predict_frames(frames.flip(1).flip(2), **KW)
        assert all(torch.equal(g.bboxes[:, 4], t.bboxes[:, 4]) for g, t in zip(both, turned))


def test_augmented_rotated_nms_and_wbf(detector, monkeypatch):
    from mydetection_amd import ops
    from mydetection_amd.api import Augment, Nms, Tiles
    name, det = detector
    frames = torch.from_numpy(_synthetic_frames(B, H, W, seed=70)).cuda()
    with pytest.raises(ValueError, match='tiled'):
        det.predict_frames(frames, augment=Augment(), tiles=Tiles((96, 128)), **KW)
    calls = []
    real = ops.fuse_view_records
    monkeypatch.setattr(ops, 'fuse_view_records', lambda *a, **k: (calls.append((a, k)), real(*a, **k))[1])
    if name == 'rapid':
        with pytest.raises(ValueError, match='wbf'):
            det.predict_frames(frames, augment=Augment(fuse='wbf'), **KW)
        got = det.predict_frames(frames, augment=Augment(vflip=True), rotated_nms=True, **KW)
        assert calls[0][0][6:9] == ('nms', 'iou', True)
        want = _expected(det, frames, [0, 1, 2, 3], fuse_kw=dict(rotated_nms=True), rotated_nms=True)
        _assert_objects_equal_records(got, want, (H, W))
        return
    with pytest.raises(ValueError, match='cxcywhd'):
        det.predict_frames(frames, augment=Augment(), rotated_nms=True, **KW)
    aug = Augment(vflip=True, fuse='wbf', thres=0.55, min_score=0.002)
    got = det.predict_frames(frames, augment=aug, **KW)
    assert calls[0][0][2:4] == (4, [0, 1, 2, 3]) and calls[0][0][5:8] == (0.55, 'wbf', 'iou') and calls[0][0][10] == 0.002
    want = _expected(det, frames, [0, 1, 2, 3], thres=0.55, fuse_kw=dict(kind='wbf', min_score=0.002))
    assert sum(want['count'].tolist()) > 0
    _assert_objects_equal_records(got, want, (H, W))
    nms_fused = det.predict_frames(frames, augment=Augment(vflip=True, thres=0.55), **KW)
    assert _differs(got, nms_fused)                                  # means of boxes, not picks among them
    # an Nms mode runs whole in every view; the fusion takes its `agnostic`
    calls.clear()
    mode = Nms('soft-linear', agnostic=True)
    got = det.predict_frames(frames, augment=Augment(), nms=mode, **KW)
    assert calls[0][0][9]
    _assert_objects_equal_records(got, _expected(det, frames, [0, 1], fuse_kw=dict(agnostic=True), nms=mode), (H, W))


def test_augmented_yuv_equals_augmented_rgb(detector):
    from mydetection_amd import ops
    from mydetection_amd.api import Augment
    name, det = detector
    rng = np.random.Generator(np.random.PCG64(9))
    h, w = 96, 128
    rgb = _synthetic_frames(B, h, w, seed=80)
    y = torch.from_numpy((rgb.astype(np.float32) @ np.array([0.257, 0.504, 0.098], np.float32) + 16).clip(0, 255).astype(np.uint8)).cuda()
    uv = torch.from_numpy(rng.integers(64, 192, (B, h // 2, w // 2, 2), dtype=np.uint8)).cuda()
    aug = Augment(hflip=True, vflip=True)
    want = det.predict_frames(ops.yuv420_to_rgb((y, uv), 'nv12'), augment=aug, **KW)
    assert sum(len(o) for o in want) > 0
    for got in (det.predict_frames_yuv((y, uv), 'nv12', augment=aug, **KW), det.predict_frames_nv12(y, uv, augment=aug, **KW)):
        for g, o in zip(got, want):
            assert g.img_hw == o.img_hw == (h, w)
            assert torch.equal(g.bboxes, o.bboxes) and torch.equal(g.scores, o.scores) and torch.equal(g.cats, o.cats)
    eval_type = 'cxcywhd' if name == 'rapid' else 'x1y1wh'
    rows = det.frames_nv12_to_json(y, uv, [3, 4], eval_type, augment=aug, **KW)
    assert rows == [r for o, i in zip(want, (3, 4)) for r in o.to_json(i, eval_type)]


def _check_chips(det, frames, objs, got, chips):
    """chips[b][k] equals the dense call on row k of objs[b].bboxes (4 or 5 wide)."""
    from mydetection_amd import ops
    kw = chips.kwargs(det.model.input_format)
    kw.pop('max_per_frame')
    total = 0
    for b, (o, c) in enumerate(zip(objs, got)):
        n = min(len(o), chips.max_per_frame)
        assert c.shape[0] == n and c.is_cuda
        if n:
            want = ops.crop_boxes(frames[b:b + 1], o.bboxes.to('cuda', torch.float32)[None, :n], **kw)
            assert torch.equal(c, want[0]), (b, n)
        total += n
    return total


def test_tracker_drawing_and_chips_read_the_fused_records(detector):
    from mydetection_amd.api import Augment, Chips, Draw, Tracker
    name, det = detector
    frames = np.ascontiguousarray(_synthetic_frames(B, H, W, seed=70))          # packed pixels: a device tensor is drawn in place
    dev = torch.from_numpy(frames).cuda()
    aug = Augment(hflip=True)
    want = det.predict_frames(dev, augment=aug, **KW)
    assert sum(len(o) for o in want) > 0
    draw = Draw(labels=('class', 'score'), label_height=8, fill_alpha=50)
    dev_in = dev.clone()
    objs, drawn = det.annotate_frames(dev_in, draw, augment=aug, **KW)
    _same_objects(objs, want)
    assert drawn.data_ptr() == dev_in.data_ptr() and torch.equal(drawn, _drawn_from_objects(frames, want, draw.style((H, W))))
    chips = Chips(size=(32, 16), pad=1.2, max_per_frame=8)
    objs, got = det.crop_frames(dev, chips, augment=aug, **KW)
    _same_objects(objs, want)
    assert _check_chips(det, dev, objs, got, chips) > 0              # chip k is row k
    # a tracker reads the fused records as it reads any records
    both = np.stack([frames[0], frames[0]])
    trk, trk_ref = Tracker(min_score=0.0005), Tracker(min_score=0.0005)
    fused = det.predict_frames(both, augment=aug, **KW)
    for call in range(2):
        tracked = det.predict_frames(both, tracker=trk, augment=aug, **KW)
        assert all(o.obj_ids is not None for o in tracked) and sum(len(o) for o in tracked) > 0
        objs, got = det.crop_frames(both, chips, tracker=trk_ref, augment=aug, **KW)
        _same_objects(objs, tracked)
    assert len(tracked[0]) <= len(fused[0]) + len(fused[1])


def test_pil_calls_take_the_frame_path(detector):
    from mydetection_amd.api import Augment
    name, det = detector
    frames = _synthetic_frames(B, H, W, seed=70)
    other = _synthetic_frames(1, 120, 90, seed=71)
    aug = Augment(hflip=True)
    want = det.predict_frames(frames, augment=aug, **KW)
    one = det.detect_one(pil_img=PIL.Image.fromarray(frames[0]), augment=aug, **KW)
    single = det.predict_frames(frames[:1], augment=aug, **KW)[0]
    assert len(one) == len(single) > 0 and torch.equal(one.bboxes, single.bboxes) and torch.equal(one.scores, single.scores)
    assert one.img_hw == (H, W)
    imgs = [PIL.Image.fromarray(frames[0]), PIL.Image.fromarray(other[0]), PIL.Image.fromarray(frames[1])]
    got = det.predict_batch(imgs, augment=aug, **KW)                  # two image sizes: one augmented call each
    _same_objects([got[0], got[2]], want)
    assert got[1].img_hw == (120, 90) and _differs([got[1]], det.predict_batch([imgs[1]], **KW))
    _same_objects([got[1]], det.predict_frames(other, augment=aug, **KW))
    assert not _differs(det.predict_batch(imgs[:1], augment=None, **KW), det.predict_batch(imgs[:1], **KW))
