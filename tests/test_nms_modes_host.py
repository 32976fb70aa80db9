"""CPU: the rules of the NMS modes (include/mydet.h, "NMS modes") as tests/_nms_ref.py restates them, on cases small enough to
work out by hand; the argument rules of mydetection_amd.api.Nms and of every `nms=` entry, which touch no device; the C ABI's
new names; and the seed condition that lets tests/test_gpu_nms_modes.py compare the Gaussian kind with `==`."""
import os
import re

import numpy as np
import pytest
import torch

import _nms_cases as nc
import _nms_ref as ref
from mydetection_amd import ops
from mydetection_amd.api import Nms

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# A and B overlap: A = [0,20] x [0,20], B = [2,22] x [0,20]: inter 18 * 20 = 360, union 400 + 400 - 360 = 440.  C is apart.
A, B_, C = (10, 10, 20, 20), (12, 10, 20, 20), (100, 10, 20, 20)
O_AB = F32(360) / F32(440)


def _run(boxes, cls, scores, kind, **kw):
    kw.setdefault('conf', 0.25)
    kw.setdefault('thr', 0.45)
    conf, thr = kw.pop('conf'), kw.pop('thr')
    return ref.run(np.asarray(boxes, F32), np.asarray(cls, np.int64), np.asarray(scores, F32), conf, thr, kind, **kw)


def test_pair_value_by_hand():
    o = ref.pair_matrix(np.asarray([A, B_, C], F32))
    assert o[0, 1].view(np.uint32) == O_AB.view(np.uint32) and o[1, 0] == o[0, 1] and o[0, 2] == 0 and o[0, 0] == 1
    z = ref.pair_matrix(np.asarray([(5, 5, 0, 0), (5, 5, 0, 0)], F32))
    assert np.isnan(z[0, 1])                                      # 0 / 0


def test_soft_linear_reorders_and_keeps_the_decayed_bits():
    out = _run([A, B_, C], [0, 0, 0], [0.9, 0.8, 0.7], 'soft-linear', conf=0.1)      # min_score = conf = 0.1
    assert out['index'].tolist() == [0, 2, 1]                     # A, then C: B fell to 0.8 * (1 - 0.818) = 0.145, below C's 0.7
    want = F32(0.8) * (F32(1) - O_AB)
    assert out['score'].view(np.uint32).tolist() == [F32(0.9).view(np.uint32), F32(0.7).view(np.uint32), want.view(np.uint32)]
    assert out['score'].dtype == F32 and np.array_equal(out['bbox'], np.asarray([A, C, B_], F32))


def test_min_score_cuts_the_rest_of_the_group():
    out = _run([A, B_, C], [0, 0, 0], [0.9, 0.8, 0.7], 'soft-linear')          # min_score = conf = 0.25 > 0.145
    assert out['count'] == 2 and out['index'].tolist() == [0, 2]
    out = _run([A, B_, C], [0, 0, 0], [0.9, 0.8, 0.7], 'soft-linear', min_score=0.75)
    assert out['index'].tolist() == [0]                           # C's 0.7 stops the group; B is never looked at
    out = _run([A, B_, C], [0, 0, 0], [0.9, 0.8, 0.7], 'soft-linear', min_score=0.95)
    assert out['count'] == 0 and out['bbox'].shape == (0, 4)


def test_a_tie_after_decay_goes_to_the_lower_index():
    left, right = (8, 10, 20, 20), (12, 10, 20, 20)               # mirror images about A: the same o with A
    for boxes in ([A, left, right], [A, right, left]):
        out = _run(boxes, [0, 0, 0], [0.9, 0.8, 0.8], 'soft-linear', min_score=0.0)
        assert out['index'].tolist() == [0, 1, 2], 'the candidate index decides, not the geometry'
        assert out['score'][1].view(np.uint32) == (F32(0.8) * (F32(1) - O_AB)).view(np.uint32)
    out = _run([A, left, right], [0, 0, 0], [0.9, 0.8, 0.8], 'soft-gaussian', min_score=0.0, sigma=0.5)
    w = F32(np.exp(-(np.float64(O_AB) * np.float64(O_AB)) / 0.5))
    assert out['index'].tolist() == [0, 1, 2] and out['score'][1].view(np.uint32) == (F32(0.8) * w).view(np.uint32)


def test_agnostic_joins_two_classes_on_one_box():
    boxes, cls, s = [A, A, C], [3, 1, 1], [0.9, 0.8, 0.7]
    assert _run(boxes, cls, s, 'hard')['index'].tolist() == [1, 2, 0]                       # class 1 first; both copies of A live
    out = _run(boxes, cls, s, 'hard', agnostic=True)
    assert out['index'].tolist() == [2, 0] and out['cls'].tolist() == [1, 3]                # one A, output still class ascending
    out = _run(boxes, cls, s, 'soft-linear', agnostic=True, min_score=0.0)
    assert out['index'].tolist() == [2, 1, 0] and out['score'][1] == 0                      # o = 1: the copy decays to 0 * 0.8


def test_merge_of_two_boxes_by_hand():
    out = _run([A, B_, C], [0, 0, 0], [0.9, 0.6, 0.7], 'merge')
    assert out['index'].tolist() == [0, 2] and out['score'].view(np.uint32).tolist() == [F32(0.9).view(np.uint32), F32(0.7).view(np.uint32)]
    sa, sb = float(F32(0.9)), float(F32(0.6))
    W = sa + sb
    x1, x2 = (sa * 0.0 + sb * 2.0) / W, (sa * 20.0 + sb * 22.0) / W
    y1, y2 = (sa * 0.0 + sb * 0.0) / W, (sa * 20.0 + sb * 20.0) / W
    want = np.asarray([F32((x1 + x2) * 0.5), F32((y1 + y2) * 0.5), F32(x2 - x1), F32(y2 - y1)], F32)
    assert np.array_equal(out['bbox'][0].view(np.uint32), want.view(np.uint32))
    assert abs(float(out['bbox'][0, 0]) - 10.8) < 1e-5                                      # 10 + 2 * 0.6 / 1.5
    assert np.array_equal(out['bbox'][1], np.asarray(C, F32))                               # a cluster of one is the box itself


def test_hard_without_agnostic_is_the_oracle():
    from oracle import postprocess as pp
    for seed in range(6):
        img = nc.clustered('x', 700 if seed % 2 else 200, 900 + seed, (0, 1, 2, 4095))
        out = ref.run(img['b'], img['c'], img['s'], nc.CONF, nc.THR, 'hard')
        ob, oc, os_, src = pp.post_process(img['b'], img['c'], img['s'], nc.CONF, nc.THR)
        assert out['count'] == len(src) and np.array_equal(out['index'], src) and np.array_equal(out['cls'], oc)
        assert np.array_equal(out['score'].view(np.uint32), os_.view(np.uint32)) and np.array_equal(out['bbox'], ob)


def test_every_kind_meets_its_branch_in_the_gpu_cases():
    """What tests/test_gpu_nms_modes.py asserts again before it launches: the cases re-order, cut, merge and cross classes."""
    nc.check_branches()


@pytest.mark.parametrize('name', nc.NAMES)
def test_seed_condition_for_the_gaussian_weights(name):
    """Every Gaussian weight of the launch, in float64, lies farther than 2^-45 relative from a float32 rounding midpoint: two
    correct exp implementations differ by an ulp of float64 (2^-52), so both round to the same float32 and `==` on the device is
    legitimate.  If this fails for a seed, change the seed in tests/_nms_cases.py; do not relax the comparison."""
    for agn in (False, True):
        st = nc.expected(name, 'soft-gaussian', agn)[1]
        assert st.midpoint > 2.0 ** -45, (name, agn, st.midpoint)
    print(name, 'weights', st.weights, 'midpoint distance', st.midpoint, 'smallest pick gap', st.gap)


def test_midpoint_distance():
    lo, hi = np.float64(F32(0.75)), np.float64(np.nextafter(F32(0.75), F32(1)))
    assert ref.midpoint_distance((lo + hi) / 2) == 0
    assert abs(ref.midpoint_distance(lo) - (hi - lo) / 2 / lo) < 1e-20
    assert ref.midpoint_distance(np.float64(1.0)) > 2.0 ** -26                              # 1.0: half an ulp below it at least


# --------------------------------------------------------------------------------------------------------------- the settings object
def test_nms_settings_object():
    assert Nms is ops.Nms
    n = Nms()
    assert (n.kind, n.agnostic, n.sigma, n.min_score) == ('hard', False, 0.5, None) and n.plain
    assert not Nms(agnostic=True).plain and not Nms('merge').plain
    assert repr(Nms('soft-gaussian', True, 0.3, 0.1)) == "Nms('soft-gaussian', agnostic=True, sigma=0.3, min_score=0.1)"
    assert eval(repr(Nms('soft-linear', min_score=0.2))) == Nms('soft-linear', min_score=0.2)
    assert Nms('merge') == Nms('merge', False, 0.5) and hash(Nms('merge')) == hash(Nms('merge', agnostic=0))
    assert Nms('merge') != Nms('merge', agnostic=True) and Nms('soft-gaussian') != Nms('soft-gaussian', sigma=0.25)
    assert Nms() != 'hard' and len({Nms(), Nms('hard'), Nms(agnostic=True)}) == 2
    for bad in (dict(kind='soft'), dict(kind=None), dict(kind=1), dict(agnostic='yes'), dict(agnostic=2), dict(sigma=0), dict(sigma=-1),
                dict(sigma=float('nan')), dict(sigma=float('inf')), dict(sigma='x'), dict(min_score=-0.1), dict(min_score=float('nan')),
                dict(min_score=float('inf'))):
        with pytest.raises(ValueError):
            Nms(**bad)
    with pytest.raises(AttributeError):
        n.kind = 'merge'


def test_mode_rules_raise_before_any_device():
    """CPU tensors: a call that got as far as the device check would raise RuntimeError (no CPU path), not these."""
    from mydetection_amd.utils.structures import ImageObjects, batched_post_process
    b4, b5 = torch.zeros(1, 8, 4), torch.zeros(1, 8, 5)
    c, s = torch.zeros(1, 8, dtype=torch.int64), torch.ones(1, 8)
    for fn in (ops.postprocess, ops.postprocess_dense, batched_post_process):
        for mode in (Nms(agnostic=True), Nms('soft-linear'), Nms('soft-gaussian')):
            with pytest.raises(ValueError, match='rotated_nms'):
                fn(b5, c, s, 0.3, 0.45, rotated_nms=True, nms=mode)
        with pytest.raises(ValueError, match='cxcywhd'):
            fn(b5, c, s, 0.3, 0.45, nms=Nms('merge'))
        with pytest.raises(ValueError, match='conf_thres > 0'):
            fn(b4, c, s, 0.0, 0.45, nms=Nms('merge'))
        with pytest.raises(ValueError, match='conf_thres >= 0'):
            fn(b4, c, s, -0.1, 0.45, nms=Nms('soft-linear'))
        with pytest.raises(ValueError, match='conf_thres >= 0'):
            fn(b4, c, s, float('nan'), 0.45, nms=Nms('soft-gaussian'))
        with pytest.raises(TypeError):
            fn(b4, c, s, 0.3, 0.45, nms='soft-linear')
    with pytest.raises(ValueError, match='rotated_nms'):
        ops.merge_tile_records(torch.zeros(2, ops._lib.REC_ROT_WORDS, dtype=torch.int32), 1, 2, [(0, 0), (4, 0)], 0.45,
                               rotated_nms=True, agnostic=True)
    rot = ImageObjects(torch.zeros(3, 5), torch.zeros(3, dtype=torch.int64), None, torch.ones(3), 'cxcywhd', img_hw=(8, 8))
    with pytest.raises(ValueError, match='cxcywhd'):
        rot.post_process(0.3, 0.45, nms=Nms('merge'))
    with pytest.raises(ValueError, match='rotated_nms'):
        rot.post_process(0.3, 0.45, rotated_nms=True, nms=Nms('soft-linear'))
    with pytest.raises(ValueError, match='conf_thres'):
        rot.nms(0.45, nms=Nms('soft-linear'))                     # every box is a candidate there: no threshold to decay towards
    # the mode struct: min_score defaults to the call's conf_thres
    m = ops.nms_mode('x', Nms('soft-gaussian', True, 0.25), 0.3, 4)
    assert (m.kind, m.agnostic, m.sigma, m.min_score) == (ops._lib.NMS_SOFT_GAUSSIAN, 1, 0.25, np.float32(0.3))
    assert ops.nms_mode('x', None, 0.3, 4) is None and ops.nms_mode('x', Nms(), 0.3, 5, rotated_nms=True) is None
    assert ops.nms_mode('x', Nms('soft-linear', min_score=0.5), 0.3, 5).min_score == 0.5


def test_detector_settings_raise_before_any_device():
    from mydetection_amd.api import Detector, Tiles

    class Model:
        bb_format = 'cxcywhd'
    det = Detector.__new__(Detector)
    det.model, det.rotated_nms, det.conf_thres, det.nms_thres, det.preprocess, det.input_size, det.nms = Model(), False, 0.3, 0.45, 'x', 64, None
    with pytest.raises(ValueError, match='cxcywhd'):
        det._call_settings(dict(nms=Nms('merge')))
    with pytest.raises(ValueError, match='rotated_nms'):
        det._call_settings(dict(nms=Nms(agnostic=True), rotated_nms=True))
    with pytest.raises(ValueError, match='rotated_nms'):
        det._call_settings(dict(nms=Nms('soft-linear'), rotated_nms=True, tiles=Tiles(32)))
    with pytest.raises(TypeError):
        det._call_settings(dict(nms='merge'))
    with pytest.raises(ValueError, match='conf_thres >= 0'):
        det._call_settings(dict(nms=Nms('soft-linear'), conf_thres=-1.0))
    call = det._call_settings(dict(nms=Nms('soft-linear', agnostic=True)))
    assert call.nms == Nms('soft-linear', True) and det._call_settings({}).nms is None
    det.nms = Nms(agnostic=True)                                  # the detector's default; a call's keyword overrides it
    assert det._call_settings({}).nms == Nms(agnostic=True) and det._call_settings(dict(nms=None)).nms is None
    with pytest.raises(ValueError, match='cxcywhd'):
        list(det._records_by_size([], nms=Nms('merge')))


# ------------------------------------------------------------------------------------------------------------------------- the C ABI
NEW_SYMBOLS = ('mydet_postprocess_nms_f32', 'mydet_postprocess_records_nms_f32', 'mydet_postprocess_rot_nms_f32',
               'mydet_postprocess_records_rot_nms_f32', 'mydet_merge_tile_records_nms_f32')


def test_new_symbols_are_declared_and_bound():
    from mydetection_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'mydet.h')).read()
    for name in NEW_SYMBOLS:
        assert re.search(r'\bint %s\(' % name, header), f'{name} is not declared in include/mydet.h'
        assert name in _lib.SIGNATURES
        old = name.replace('_nms_f32', '_f32')
        assert len(_lib.SIGNATURES[name]) == len(_lib.SIGNATURES[old]) + 1                   # the mode pointer / the agnostic flag
    assert re.search(r'#define MYDET_ABI_VERSION 2\b', header) and _lib.ABI_VERSION == 2
    for k, name in enumerate(('HARD', 'SOFT_LINEAR', 'SOFT_GAUSSIAN', 'MERGE')):
        assert re.search(r'#define MYDET_NMS_%s\s+%d\b' % (name, k), header) and getattr(_lib, 'NMS_' + name) == k
    assert 'typedef struct mydet_nms_mode' in header
    import ctypes
    assert ctypes.sizeof(_lib.NmsMode) == 24 and _lib.NmsMode.sigma.offset == 8 and _lib.NmsMode.min_score.offset == 16
