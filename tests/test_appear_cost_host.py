"""CPU tests of the fused IoU-and-appearance cost (mydet_track_frames_appear_optimal_f32): the declarations, exports and
bindings, the argument rules of every layer (none of them needs a device), and -- on the restatement tests/_appear_cost_ref.py
alone -- what the GPU tests of tests/test_gpu_appear_cost.py rely on: the margins of every case and the outcome it is for."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import _appear_cost_cases as cases
import _appear_cost_ref as ref
import _appear_ref
import _assoc_ref
import _track_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('mydet_track_frames_appear_optimal_f32', 'mydet_track_appear_ws_words')


def test_entry_points_are_declared_exported_and_bound():
    from mydetection_amd import _lib, ops
    header = open(os.path.join(ROOT, 'include', 'mydet.h')).read()
    design = open(os.path.join(ROOT, 'DESIGN.md')).read()
    dll = ctypes.CDLL(_lib.LIB_PATH)
    for name, nargs in zip(NAMES, (26, 1)):
        assert re.search(r'\b(int|int64_t)\s+' + name + r'\s*\(', header)
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name]) == nargs
        assert hasattr(dll, name)
        assert getattr(_lib.lib(), name).argtypes == _lib.SIGNATURES[name]
    assert _lib.lib().mydet_track_appear_ws_words.restype == ctypes.c_int64
    for mt in (1, 63, 64, 65, 512):
        assert _lib.lib().mydet_track_appear_ws_words(mt) == ops.appear_ws_words(mt) == 512 * mt
    assert _lib.lib().mydet_track_appear_ws_words(0) == 0 and _lib.lib().mydet_track_appear_ws_words(513) == 0
    for mt in (0, 513):
        with pytest.raises(ValueError, match='max_tracks'):
            ops.appear_ws_words(mt)
    # the rule text: the cost, the workspace contract, the refusals -- in the header and in the design document
    for text in ('m = ((256 - weight) * q + weight * a) >> 8', 'sim_ws[d * MT + j] == S(j, d)', 'mydet_track_appear_ws_words'):
        assert text in header and text in design, text
    for text in ('q = (int)floorf(iou * 65536.0f)', 'a = S >> 1', 'weight outside 0..256', 'the walk\'s key stays IoU-major',
                 'None of that depends on the solver\'s outcome'):
        assert text in header, text
    mk = open(os.path.join(ROOT, 'mydetection_amd', 'csrc', 'Makefile')).read()
    assert re.search(r'SRCS_EXACT\s*=.*\btrack_appear_optimal\.hip\b', mk)


def test_c_entry_point_checks_its_arguments_before_any_launch():
    """Every call below must fail its checks: the pointers are never dereferenced, no device is needed."""
    from mydetection_amd import _lib, ops
    par, aset = ops.track_params((480, 640)), ops.appear_set()
    P = 0x10000                                                      # aligned, never read

    def call(assoc=None, weight=128, ws=P, aset=aset, mt=64, desc=P, astate=P, records=P):
        assoc = ops.track_assoc('optimal') if assoc is None else assoc
        return _lib.lib().mydet_track_frames_appear_optimal_f32(records, 0, 0, 1, 1, 4, ctypes.byref(par), mt, P, P, P, P, P, P, P, P,
                                                                ctypes.byref(assoc), None, ctypes.byref(aset), desc, astate, P, P, weight, ws, None)
    assert call(assoc=ops.track_assoc('greedy')) == -2
    assert call(assoc=ops.track_assoc('greedy', 0.2, 0.5, 0.3)) == -2
    for w in (-1, 257, 1 << 20):
        assert call(weight=w) == -1
    assert call(ws=None) == -1 and call(ws=P + 4) == -1 and call(ws=P + 8) == -1
    # everything mydet_track_frames_appear_f32 refuses
    assert call(desc=None) == -1 and call(astate=P + 4) == -1 and call(records=None) == -1 and call(mt=0) == -1 and call(mt=513) == -2
    for field, v in (('alpha', 0), ('alpha', 257), ('gate', -1), ('gate', 131073), ('reid', 131073), ('reach', -1.0), ('reach', float('inf')),
                     ('update_thres', float('nan'))):
        bad = ops.appear_set()
        setattr(bad, field, v)
        assert call(aset=bad) == -1, (field, v)
    # a refused weight or workspace comes before the greedy refusal; the other entry point still refuses the optimal assignment
    assert call(assoc=ops.track_assoc('greedy'), weight=300) == -1
    assert _lib.lib().mydet_track_frames_appear_f32(P, 0, 0, 1, 1, 4, ctypes.byref(par), 64, P, P, P, P, P, P, P, P,
                                                    ctypes.byref(ops.track_assoc('optimal')), None, ctypes.byref(aset), P, P, P, P, None) == -2


def test_ops_and_api_refusals_need_no_device():
    from mydetection_amd import _lib, ops
    from mydetection_amd.api import Appearance, Tracker
    rec = torch.zeros((1, _lib.REC_WORDS), dtype=torch.int32)
    state = torch.zeros((1, ops.track_state_words(64)), dtype=torch.int32)
    par = ops.track_params((480, 640))
    ap = (ops.appear_set(), torch.zeros((1, 512, 128), dtype=torch.uint16), torch.zeros((1, ops.appear_state_words(64)), dtype=torch.int32))
    ws = torch.zeros((1, ops.appear_ws_words(64)), dtype=torch.int32)
    for assoc in (None, ops.track_assoc('greedy'), ops.track_assoc('greedy', 0.2, 0.5, 0.3)):
        with pytest.raises(ValueError, match="assign 'optimal' only"):
            ops.track_frames(rec, state, par, assoc=assoc, appear=ap, appear_weight=128, appear_ws=ws)
    for w in (-1, 257, 0.5, True, '1'):
        with pytest.raises(ValueError, match='0..256'):
            ops.track_frames(rec, state, par, assoc=ops.track_assoc('optimal'), appear=ap, appear_weight=w, appear_ws=ws)
    with pytest.raises(ValueError, match='appear='):
        ops.track_frames(rec, state, par, assoc=ops.track_assoc('optimal'), appear_weight=128, appear_ws=ws)
    with pytest.raises(ValueError, match='appear_weight'):
        ops.track_frames(rec, state, par, appear=ap, appear_ws=ws)
    # without a weight every refusal is today's
    with pytest.raises(ValueError, match="assign 'greedy' only"):
        ops.track_frames(rec, state, par, assoc=ops.track_assoc('optimal'), appear=ap)
    with pytest.raises(ValueError, match='streams'):
        ops.appear_workspace(0, 64, 'cpu')
    assert ops.appear_workspace(2, 65, 'cpu').shape == (2, 512 * 65) and ops.appear_workspace(2, 65, 'cpu').dtype == torch.int32

    for w in (-0.01, 1.01, float('nan'), 128):
        with pytest.raises(ValueError, match='weight'):
            Appearance(weight=w)
    assert [Appearance(weight=w).weight256 for w in (0, 0.001, 0.002, 0.5, 0.998, 1)] == [0, 0, 1, 128, 255, 256]
    assert Appearance().weight is None and Appearance().launch_args() == {}
    assert repr(Appearance()) == 'Appearance(gate=0.3, reid=0.6, momentum=0.9, reach=2.0, update_thres=None)'
    assert repr(Appearance(weight=0.5)) == 'Appearance(gate=0.3, reid=0.6, momentum=0.9, reach=2.0, update_thres=None, weight=0.5)'
    with pytest.raises(ValueError, match="assign='optimal'"):
        Appearance(weight=0.5).check_tracker(Tracker())
    with pytest.raises(ValueError, match='greedy'):
        Appearance().check_tracker(Tracker(assign='optimal'))
    Appearance(weight=0.5).check_tracker(Tracker(assign='optimal'))
    Appearance().check_tracker(Tracker())


def test_the_affinity_is_the_rule_text():
    assert ref.affinity(40000, 131072, 1, 0) == 40000 and ref.affinity(40000, 131072, 1, 256) == 65536
    assert ref.affinity(40000, 100001, 1, 128) == (128 * 40000 + 128 * 50000) >> 8 and ref.affinity(40000, 100001, 0, 256) == 40000
    assert ref.affinity(1, 1, 1, 255) == 0                            # the shift floors
    c = ref.cost_matrix(np.array([[10, 0], [65536, 7]]), np.array([[True, False], [True, True]]))
    assert c.tolist() == [[65526, 131072, 65536, 65536], [0, 65529, 65536, 65536]]


def test_the_swap_on_the_restatements():
    """Case 1 on the CPU: the optimal assignment on IoU alone swaps the ids, the fused cost keeps them; in the second scene the
    greedy walk with the default gate gives the neighbour's track away and the fused assignment does not."""
    for neighbour in (False, True):
        frames, descs = cases.swap(4, neighbour)
        plain = _assoc_ref.Stream(64, _track_ref.Params(cases.TRACK_HW, np.float32), assign='optimal')
        outs = [plain.step(*_track_ref.unpack_frame(r, 4)) for r in _track_ref.pack_records(frames, 4)]
        assert _assoc_ref.margins_hold(plain) and outs[3]['match'][:2] == [0, 1] and outs[3]['id'][:2] == [1, 2]     # each track took the OTHER object
        _, _, stream, fused, _ = cases.restated('swap', neighbour, 128)
        assert ref.margins_hold(stream) and fused[3]['match'][:2] == [1, 0] and fused[3]['id'][:2] == [1, 2] and fused[3]['how'][:2] == [1, 1]
        assert fused[3]['sim'][:2] == [131072, 131072]
    frames, descs = cases.swap(4, True)
    greedy, outs, _ = _appear_ref.run(frames, descs, 4, cases.TRACK_HW, 64, appear=dict(gate=cases.level(0.3)))
    assert outs[3]['match'][:2] == [0, 1] and outs[3]['sim'][:2] == [65536, 65536]                  # passed the gate, swapped
    m = greedy.margins
    assert m['iou_thres'] >= 0.05 and m['iou_gap'] >= 0.05 and m['sim'] > 0
    # weight 0 in that scene is the IoU assignment again: the gate lets the swapped pairs through
    _, _, stream, outs, _ = cases.restated('swap', True, 0)
    assert ref.margins_hold(stream) and outs[3]['match'][:2] == [0, 1]


def test_the_painted_swap_on_the_restatements():
    frames, recs = cases.painted_swap()
    boxes = np.zeros((4, 512, 5), np.float32)
    for f, r in enumerate(recs):
        boxes[f, :2] = r[0]
    desc, info = _appear_ref.descriptors(frames, boxes, np.array([2] * 4))
    assert all(i['u'] == 0 for row in info for i in row[:2])         # angle 0: every sample is settled
    appear = dict(gate=cases.level(0.3), reid=cases.level(0.6), alpha=_appear_ref.alpha_of(0.9), reach=2.0, update_thres=0.3)
    got = {}
    for weight in (0, 128):
        stream, outs, _ = ref.run(recs, desc, 5, frames.shape[1:3], 64, params=dict(match='rotated'), appear=appear, weight=weight)
        assert ref.margins_hold(stream), stream.margins
        got[weight] = outs[3]['match'][:2]
    assert got == {0: [1, 0], 128: [0, 1]}                            # record slot 0 is the first object here


@pytest.mark.parametrize('mt', sorted(cases.GRID_NS))
def test_the_shape_cases_hold_their_margins(mt):
    frames, descs, stream, outs, arrays = cases.restated('grid', mt)
    ns = cases.GRID_NS[mt]
    assert len(frames) == 4 and ref.margins_hold(stream), stream.margins
    assert [len(fr[1]) for fr in frames] == list(ns)
    for f in range(1, 4):
        matched = [k for k, h in enumerate(outs[f]['how']) if h == 1]
        assert len(matched) == min(ns[f], outs[f - 1]['count']) and all(outs[f]['sim'][k] > 100000 for k in matched)      # a template update in every frame
        assert not np.array_equal(arrays[f]['tmpl'], arrays[f - 1]['tmpl']) or not matched
        # every track born in frame f - 1 and seen again decides with its own template: its pair is matched with S of the birth
        for k, h in enumerate(outs[f - 1]['how']):
            if h == 4 and outs[f]['how'][k] == 1:
                assert outs[f]['sim'][k] > 100000
    if mt == 1:
        assert [o['dropped'] for o in outs] == [0, 1, 0, 0] and outs[2]['how'] == [0]                 # a live track and no detections
    if mt == 64:
        assert outs[2]['dropped'] == 1 and outs[3]['how'].count(0) == 64
    if mt == 512:
        # the visibility hazard: a track in a slot >= 64, born in the frame before, matched with a detection whose S another wave computed
        nwave = 8
        hit = [(k, d) for k, (h, d) in enumerate(zip(outs[2]['how'], outs[2]['match'])) if h == 1 and k >= 64 and outs[1]['how'][k] == 4 and
               d % nwave != k // 64]
        assert len(hit) > 100
        assert len(stream.needed) >= 63


def test_the_crowd_needs_the_dense_form():
    frames, descs, stream, outs, arrays = cases.restated('crowd')
    assert ref.margins_hold(stream), stream.margins
    assert outs[0]['how'][70:90] == [4] * 20
    for f, k in ((1, 7), (2, 12), (3, 3)):
        how = outs[f]['how'][70:90]
        assert how[k] == 1 and how.count(0) == 19 and outs[f]['sim'][70 + k] > 100000
    d = 70                                                            # the crowd's one detection: 20 needed pairs in slots 64 .. 127
    assert sorted(k for (dd, k) in stream.needed if dd == d) == list(range(70, 90))


@pytest.mark.parametrize('key', cases.SETTINGS, ids=lambda k: '-'.join(str(v) for v in k))
def test_the_settings_cases_hold_their_margins(key):
    variant, bands, shift, gate, reid, weight = key
    frames, descs, stream, outs, arrays = cases.restated('settings', *key)
    assert ref.margins_hold(stream), stream.margins
    hows = {h for o in outs for h in o['how']}
    assert hows >= {-1, 0, 1, 4} and (2 in hows) == bands and (3 in hows) == (reid > 0)
    assert outs[3]['count'] == _track_ref.BAD_CLASS
    if gate:                                                          # the pair only the gate removes: the track stays unmatched, the detection is born
        slot = outs[0]['how'].index(4, 6)
        assert slot == 6 and [o['how'][6] for o in outs] == [4, 1, 1, -1, 1, 0, 0] and outs[5]['how'].count(4) >= 2
    if bands:                                                         # the low duplicate beside object 0: needed, and never matched
        dup = len(frames[6][1]) - 1
        assert (dup, 0) in stream.needed and dup not in outs[6]['match'] and outs[6]['how'][0] == 1


def test_weight_zero_is_the_plain_optimal_assignment_on_the_restatements():
    for variant, bands in (('bw4', False), ('rot', True)):
        key = (variant, bands, False, 0.0, 0.0, 0)
        frames, descs, stream, outs, arrays = cases.restated('settings', *key)
        v = cases.VARIANTS[variant]
        par = _track_ref.Params(cases.TRACK_HW, np.float32, match=v['match'])
        plain = _assoc_ref.Stream(64, par, assign='optimal', **(cases.BANDS if bands else {}))
        want = [plain.step(*_track_ref.unpack_frame(r, v['width'])) for r in _track_ref.pack_records(frames, v['width'])]
        for o, w in zip(outs, want):
            assert all(o[k] == w[k] for k in ('id', 'missed', 'match', 'count', 'dropped'))
