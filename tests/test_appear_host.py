"""CPU-only: the host side of the appearance -- properties of the restatement (tests/_appear_ref.py), the template arithmetic at
its edges, the settled conditions on the cases of tests/_appear_cases.py that keep the comparison of tests/test_gpu_appear.py from
being hollow, the same for every case of tests/test_gpu_appear_branches.py (the outcome it is for occurs, the margins hold, and the
restatement with that one rule altered gives other outputs), the C ABI (declared, exported, bound, constants, the ABI version unchanged, argument checks before any launch) and
the argument rules of ops.appear_* and api.Appearance."""
import ctypes
import inspect
import os
import re
import textwrap

import numpy as np
import pytest
import torch

import _appear_cases as cases
import _appear_ref as ref
import _yuv420_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('mydet_appear_boxes_rgb_u8', 'mydet_appear_boxes_yuv420', 'mydet_track_frames_appear_f32', 'mydet_track_appear_state_words')


def _two_tone(top, bottom, H=40, W=40):
    img = np.zeros((H, W, 3), np.uint8)
    img[:H // 2], img[H // 2:] = top, bottom
    return img


def _bin(half, rgb):
    return half * 64 + (rgb[0] >> 6) * 16 + (rgb[1] >> 6) * 4 + (rgb[2] >> 6)


def test_descriptor_properties():
    red, blue = (255, 10, 10), (10, 10, 255)
    one = ref.describe(_two_tone(red, red), [20, 20, 16, 24, 0])['desc']
    assert one.sum() == 512 and one[_bin(0, red)] == 256 and one[_bin(1, red)] == 256 and np.count_nonzero(one) == 2
    two = ref.describe(_two_tone(red, blue), [20, 20, 16, 24, 0])['desc']
    assert two[_bin(0, red)] == 256 and two[_bin(1, blue)] == 256 and np.count_nonzero(two) == 2
    turned = ref.describe(_two_tone(red, blue), [20, 20, 16, 24, 180])['desc']
    assert turned[_bin(0, blue)] == 256 and turned[_bin(1, red)] == 256 and np.count_nonzero(turned) == 2
    # a box outside the frame reads edge pixels: here the top left corner, for every sample
    img = _two_tone(red, blue)
    img[0, 0] = (70, 140, 210)
    out = ref.describe(img, [-50, -60, 16, 24, 0])['desc']
    assert out[_bin(0, (70, 140, 210))] == 256 and out[_bin(1, (70, 140, 210))] == 256
    for row in ([float('nan'), 20, 16, 24, 0], [20, 20, 16, float('nan'), 0], [20, 20, 16, 24, float('nan')], [20, 20, float('inf'), 24, 0]):
        assert ref.describe(img, row)['desc'].sum() == 0, row
    # the central 0.75: a frame of another colour around the box's inner part is not seen
    ring = _two_tone(red, red)
    ring[:, :14], ring[:, 26:] = (0, 255, 0), (0, 255, 0)
    assert np.array_equal(ref.describe(ring, [20, 20, 16, 24, 0])['desc'], one)


def test_420_restatement_is_the_rgb_one_on_the_converted_frames():
    planes = _yuv420_ref.random_planes('nv12', 2, 48, 66, seed=8)
    rgb = _yuv420_ref.to_rgb(planes, 'nv12', 'bt709', True)
    assert rgb.shape == (2, 48, 66, 3) and rgb.dtype == np.uint8
    boxes, counts = cases.boxes()
    desc, _ = ref.descriptors(rgb, boxes, counts)
    for layout in ('i420', 'p010'):
        other = _yuv420_ref.from_nv12(*planes, layout, seed=3)
        again, _ = ref.descriptors(_yuv420_ref.to_rgb(other, layout, 'bt709', True), boxes, counts)
        assert np.array_equal(desc, again)
    assert desc[1, counts[1]:].sum() == 0 and desc[0].sum() > 0


def test_template_arithmetic_at_its_edges():
    assert ref.blend(1000, 3, 256) == 768                            # alpha 256: the template becomes 256 * d
    assert ref.blend(0, 512, 256) == ref.SIM_MAX and ref.blend(ref.SIM_MAX, 0, 256) == 0
    assert ref.blend(0, 1, 1) == 1 and ref.blend(0, 512, 1) == 512   # alpha 1: 1/256 of the difference
    assert ref.blend(256, 0, 1) == 255 and ref.blend(255, 0, 1) == 254            # -255 / 256 floors to -1, not to 0
    assert ref.blend(1, 0, 1) == 0 and ref.blend(1, 0, 128) == 0     # a negative difference floors: the template reaches 0
    assert ref.blend(100, 0, 26) == 100 + ((-100 * 26) >> 8) == 89
    assert ref.alpha_of(0.9) == 26 and ref.alpha_of(0.0) == 256 and ref.alpha_of(0.5) == 128
    assert ref.level(0.3) == 39322 and ref.level(0.6) == 78643 and ref.level(1.0) == ref.SIM_MAX and ref.level(None) == 0
    assert ref.similarity(256 * cases.RED.astype(np.int64), cases.RED) == ref.SIM_MAX
    assert ref.similarity(256 * cases.RED.astype(np.int64), cases.BLUE) == 0
    assert ref.similarity(256 * cases.RED.astype(np.int64), cases.MIXED) == ref.SIM_MAX // 2
    from mydetection_amd import ops
    s = ops.appear_set(0.3, 0.6, 0.9, 2.0, 0.25)
    assert (s.gate, s.reid, s.alpha, s.reach, s.update_thres) == (39322, 78643, 26, 2.0, 0.25)
    s = ops.appear_set(None, 0, 0.0, 0.0, float('-inf'))
    assert (s.gate, s.reid, s.alpha) == (0, 0, 256)


def test_the_cases_are_settled_enough_to_mean_something():
    """Every axis-aligned and quarter-turn box is fully settled (its float32 arithmetic is the kernel's), at least half of the
    other rotated boxes are, at least 99 % of all samples are, and every rotated box is inside the bound TOL was derived for."""
    frames = cases.frames()
    boxes, counts = cases.boxes()
    _, info = ref.descriptors(frames, boxes, counts)
    rotated, samples, unsettled = [], 0, 0
    for b in range(2):
        for k in range(int(counts[b])):
            row, i = boxes[b, k], info[b][k]
            samples += ref.SAMPLES
            unsettled += i['u']
            if not np.isfinite(row).all():
                assert i['u'] == 0 and i['desc'].sum() == 0
            elif ref.quarter(row[4]):
                assert i['u'] == 0
            else:
                assert ref.within_bound(row), row
                rotated.append(i['u'] == 0)
                assert i['settled'].sum() + i['u'] == ref.SAMPLES
    assert len(rotated) >= 8 and sum(rotated) >= len(rotated) / 2, rotated
    assert unsettled <= 0.01 * samples
    _, tiny = ref.descriptors(cases.frames()[:1], cases.tiny_boxes())
    assert all(i['u'] == 0 for i in tiny[0])
    names = dict(cases.named_rows())
    assert {'one_pixel', 'half_outside', 'outside', 'angle_0', 'angle_30', 'angle_90', 'angle_-135', 'angle_450', 'nan', 'inf'} <= set(names)


def test_scenarios_fail_without_the_appearance_and_pass_with_it():
    """On the restatement alone: (a) a lost track returns under a new id without reid and under its own with it; (b) two
    tracks swap without the gate and keep their own with it."""
    fr, ds = cases.lost_and_found()
    for reid, same in ((0, False), (ref.level(0.6), True)):
        _, outs, _ = ref.run(fr, ds, 4, cases.TRACK_HW, 64, appear=dict(reid=reid))
        ids_before, ids_after = [i for i in outs[3]['id'] if i], [i for i, m in zip(outs[8]['id'], outs[8]['missed']) if i and m == 0]
        assert ids_before == [1]
        assert ids_after == ([1] if same else [2])
        assert (3 in outs[8]['how']) == same
    fr, ds = cases.crossing()
    for gate, swapped in ((0, True), (ref.level(0.3), False)):
        _, outs, _ = ref.run(fr, ds, 4, cases.TRACK_HW, 64, appear=dict(gate=gate))
        last = outs[-1]
        red, blue = last['id'].index(1), last['id'].index(2)         # born from record slots 0 (RED) and 1 (BLUE) in frame 0
        assert (last['match'][red], last['match'][blue]) == ((0, 1) if swapped else (1, 0))       # frame 3: slot 0 is BLUE


def test_the_busy_scene_uses_every_rule():
    fr, ds = cases.busy(5, low=True, rot=True)
    s, outs, arrays = ref.run(fr, ds, 5, cases.TRACK_HW, 64, params=dict(match='rotated'),
                              appear=dict(gate=ref.level(0.3), reid=ref.level(0.5), update_thres=0.5),
                              assoc=dict(low_thres=0.2, high_thres=0.5, low_match_thres=0.3))
    hows = {h for o in outs for h in o['how']}
    assert {-1, 0, 1, 2, 3, 4} <= hows, hows
    assert outs[3]['count'] == -1 and s.margins['iou_thres'] >= 0.02 and s.margins['band'] >= 1e-3 and s.margins['score'] >= 1e-3
    assert any(len(np.unique(a['tmpl'][:, 0])) > 3 for a in arrays)  # templates blend


# ---- the cases of tests/test_gpu_appear_branches.py, on the restatement alone ----

def _altered(old, new):
    """_appear_ref.Stream with ONE rule altered: the text `old`, which must occur exactly once in step, replaced by `new`."""
    src = textwrap.dedent(inspect.getsource(ref.Stream.step))
    assert src.count(old) == 1, old
    ns = {}
    exec(compile(src.replace(old, new), '<altered step>', 'exec'), vars(ref), ns)
    return type('Altered', (ref.Stream,), {'step': ns['step']})


_M = 'm = max(x[2], x[3], boxes[d][2], boxes[d][3])'
_CAND = 'if d in match.values() or stage[d] != 1 or not scores[d] >= new32:'
ALTERED = {
    'gate >': ('if s < self.gate:', 'if s <= self.gate:'),
    'reid >': ('if s >= self.reid and', 'if s > self.reid and'),
    'missed >= 1': ('t.missed < 2', 't.missed < 1'),
    'reach <': ('<= lim and abs(boxes[d][1] - x[1]) <= lim', '< lim and abs(boxes[d][1] - x[1]) < lim'),
    'm of the detection': (_M, 'm = max(boxes[d][2], boxes[d][3])'),
    'm of the track': (_M, 'm = max(x[2], x[3])'),
    'm without track_w': (_M, 'm = max(x[3], boxes[d][2], boxes[d][3])'),
    'm without track_h': (_M, 'm = max(x[2], boxes[d][2], boxes[d][3])'),
    'm without det_w': (_M, 'm = max(x[2], x[3], boxes[d][3])'),
    'm without det_h': (_M, 'm = max(x[2], x[3], boxes[d][2])'),
    'x alone': (' and abs(boxes[d][1] - x[1]) <= lim', ''),
    'y alone': ('abs(boxes[d][0] - x[0]) <= lim and ', ''),
    'any class': ('if k in match or t.cls != cats[d] or not self.has[k]', 'if k in match or not self.has[k]'),
    'below new_thres': (_CAND, 'if d in match.values() or stage[d] != 1:'),
    'low band': (_CAND, 'if d in match.values() or stage[d] == 0 or not scores[d] >= new32:'),
}


class _RoundingTake(ref.Stream):
    """The template blend with a rounding shift in place of the floor."""

    def _take(self, k, d):
        if self.has[k]:
            self.tmpl[:, k] = [int(t) + (((256 * int(v) - int(t)) * self.alpha + 128) >> 8) for t, v in zip(self.tmpl[:, k], d)]
        else:
            super()._take(k, d)


def _summary(outs, arrays):
    return [(o['how'], o['id'], o['sim'], o['dropped']) for o in outs], [a['tmpl'].tolist() for a in arrays]


def _proves(c, what=None, **over):
    """The case gives what it expects on the restatement, with the margins of the suite; with the rule `what` altered (or the
    settings `over` replaced) the outputs differ."""
    stream, outs, arrays = cases.restate(c)
    for f, k, h in c['expect']:
        assert outs[f]['how'][k] == h, (f, k, h, outs[f]['how'][k])
    m = stream.margins
    assert m['iou_thres'] >= 0.02 and m['iou_gap'] >= 0.02 and m['score'] >= 1e-3 and m['band'] >= 1e-3 and stream.ties == 0, m
    if what is not None or over:
        cls = None if what is None else what if isinstance(what, type) else _altered(*ALTERED[what])
        _, o2, a2 = cases.restate(c, cls, **over)
        assert _summary(o2, a2) != _summary(outs, arrays), (what, over)
    return stream, outs, arrays


def test_branch_cases_streams_and_odd_slot_counts():
    from mydetection_amd import ops
    assert ops.appear_state_words(65) == 8388 != 129 * 65 and all(ops.appear_state_words(mt) == 129 * mt for mt in (64, 100, 128, 512))
    assert ops.appear_state_words(1) == 132 and ops.appear_state_words(63) == 8128 and ops.appear_state_words(130) == 16772
    assert [mt % 64 for mt in (1, 63, 65, 100, 130)].count(0) == 0                  # none fills its last wave
    for width, low, rot in ((4, False, False), (5, True, True)):
        scenes = cases.stream_scenes(width, low=low, rot=rot)
        assert len(scenes) == 3 and {len(fr) for fr, _ in scenes} == {11} and {ds.shape for _, ds in scenes} == {(11, 512, 128)}
        hows = {}
        for mt in (65, 1):
            for s, (fr, ds) in enumerate(scenes):
                stream, outs, _ = ref.run(fr, ds, width, cases.TRACK_HW, mt, params=dict(match='rotated' if rot else 'iou'),
                                          appear=dict(gate=ref.level(0.3), reid=ref.level(0.5), alpha=ref.alpha_of(0.8), update_thres=0.5),
                                          assoc=cases.BANDS if low else None)
                m = stream.margins
                assert m['iou_thres'] >= 0.02 and m['iou_gap'] >= 0.02 and m['score'] >= 1e-3 and m['band'] >= 1e-3, m
                hows[mt, s] = {h for o in outs for h in o['how']}
                if mt == 1:                                          # one slot: whoever else could be born is dropped
                    two = [f for f, r in enumerate(fr) if r is not None and (r[1] >= 0.5).sum() >= 2]
                    assert len(two) == (6, 0, 4)[s] and all(outs[f]['dropped'] >= 1 for f in two), (s, two)
                    assert all(o['count'] in (-1, 0, 1) for o in outs)
        assert hows[65, 0] >= {-1, 0, 1, 3, 4} and 3 in hows[65, 1] and hows[65, 2] >= {1, 4}, hows          # the three scenes differ


def test_branch_case_many_detections():
    for mt in (192, 64):
        c = cases.many(mt)
        stream, outs, arrays = _proves(c)
        f = cases.MANY_FRAME
        assert all(len(fr[1]) > 64 for fr in c['frames'])                             # n > nthr at MT = 64: the ballot loop goes round
        if mt == 192:
            assert outs[1]['id'][:150] == list(range(1, 151)) and outs[0]['how'][:150] == [4] * 150       # born into slots 0 .. 149 in order
            assert [outs[f]['id'][k] for k in cases.MANY_LOST] == [k + 1 for k in cases.MANY_LOST]
            assert [outs[f]['missed'][k] for k in cases.MANY_LOST] == [0, 0, 0] and [outs[f - 1]['missed'][k] for k in cases.MANY_LOST] == [2, 2, 2]
            assert outs[f]['how'].count(3) == 3 and outs[f]['how'].count(4) == 3 and all(o['dropped'] == 0 for o in outs)
            assert len({k // 64 for k in cases.MANY_LOST}) == 3                       # the winners' slots: three different waves
            # the candidates of the re-identification (unmatched, above new_thres) by rank: three different words of the mask,
            # the returning objects at or beyond rank 128
            scores = c['frames'][f][1]
            rank = {int(d): p for p, d in enumerate(np.lexsort((np.arange(len(scores)), -scores.astype(np.float64))))}
            back = [rank[d] for d in range(146, 150)]
            assert min(back) >= 128 and {rank[d] >> 6 for d in range(146, 152)} == {0, 1, 2}, rank
            # the stranger: S below reid against its old track, which stays lost
            assert ref.similarity(arrays[f - 1]['tmpl'][:, cases.MANY_STRANGER], c['descs'][f][149]) < c['appear']['reid']
            assert outs[f]['missed'][cases.MANY_STRANGER] == 3
        else:
            assert all(o['dropped'] > 0 for o in outs) and outs[0]['how'] == [4] * 64 and outs[f]['how'].count(3) == 1
            assert np.array_equal(arrays[0]['tmpl'].T, 256 * c['descs'][0][:64].astype(np.int32))   # the born slots' templates
    _proves(cases.many(192), reid=0)                                  # without the re-identification the three are born anew


def test_branch_cases_integer_levels_at_equality():
    t = cases.threshold_cases()
    assert ref.similarity(256 * cases.RED.astype(np.int64), cases.MIXED) == 65536
    for name, c in t.items():
        stream, outs, _ = _proves(c, 'gate >' if name.startswith('gate') else 'reid >') if name.endswith('65536') else _proves(c)
        assert stream.margins['sim'] == 0.5, name                     # S - level + 0.5: S == level, or one below it
        f = len(c['frames']) - 1
        assert (outs[f]['sim'][0] == 65536) == name.endswith('65536'), name
    # the low band: its own threshold and how = 2
    assert t['gate_low_65536']['expect'][0] == (1, 0, 2) and t['gate_low_65536']['assoc']['low_match_thres'] == 0.3


def test_branch_cases_gate_changes_the_outcome():
    g = cases.gate_cases()
    _, outs, _ = _proves(g['second_takes'], gate=0)
    assert outs[3]['match'][:2] == [-1, 0] and cases.restate(g['second_takes'], gate=0)[1][3]['match'][:2] == [0, -1]
    _, outs, _ = _proves(g['all_refuse'], gate=0)
    assert outs[3]['id'][:3] == [1, 2, 3]
    c = g['walk_refuses_reid_takes']
    stream, outs, _ = _proves(c, reid=0)
    assert c['appear']['reid'] <= 65536 < c['appear']['gate'] and outs[4]['sim'][0] == 65536 and outs[3]['missed'][0] == 2
    assert cases.restate(c, gate=0)[1][4]['how'][0] == 1            # the IoU passes: without the gate the walk takes it


def test_branch_cases_reid_guards():
    g = cases.guard_cases()
    _proves(g['base'], reid=0)
    _proves(g['bands_base'], reid=0)
    for name, what in (('gap_0', 'missed >= 1'), ('other_class', 'any class'), ('below_new_thres', 'below new_thres'), ('low_band', 'low band')):
        stream, outs, _ = _proves(g[name], what)
        assert 3 not in outs[-1]['how']
        assert 3 in cases.restate(g[name], _altered(*ALTERED[what]))[1][-1]['how'], name
    assert g['base']['frames'][2][1].size == 0 and len(g['gap_0']['frames']) == len(g['base']['frames']) - 1       # a gap of 1 frame, of 0


def test_branch_cases_reach():
    r = cases.reach_cases()
    for name, c in r.items():
        if name.endswith('_at'):
            _proves(c, 'reach <')
            _proves(r[name[:-3] + '_past'])
    for arg in cases.REACH_SIZES:                                    # each argument of the max decides its case
        _proves(r[arg + '_at'], 'm without ' + arg)
        for other in cases.REACH_SIZES:
            if other != arg:
                assert cases.restate(r[arg + '_at'], _altered(*ALTERED['m without ' + other]))[1][4]['how'][0] == 3
    _proves(r['track_w_at'], 'm of the detection')
    _proves(r['det_w_at'], 'm of the track')
    _proves(r['y_only_past'], 'x alone')
    _proves(r['track_w_past'], 'y alone')
    stream, outs, arrays = _proves(r['shift_at'])
    assert arrays[3]['x'][:2, 0].tolist() == [200.0, 200.0]          # the prediction is exact, and moves by (7, -3)
    c = dict(r['shift_at'], shifts=None)
    assert cases.restate(c)[1][4]['how'][:2] == [0, 4]
    assert cases.restate(dict(r['shift_past'], shifts=None))[1][4]['how'][:2] == [0, 4]
    assert r['reach_0_at']['appear']['reach'] == 0.0 and r['reach_0_past']['frames'][4][0][0, 0] == np.nextafter(np.float32(200), np.float32(201))


def test_branch_cases_templates_and_rebirth():
    t = cases.template_cases()
    _, _, a1 = _proves(t['alpha_1'], _RoundingTake)
    _, _, a256 = _proves(t['alpha_256'], alpha=255)
    assert cases.ONE[5] == 512 and cases.ONE.sum() == 512 and not cases.ZERO.any()
    seq = cases.TEMPLATE_SEQ
    for f in range(12):
        assert np.array_equal(a256[f]['tmpl'][:, 0], 256 * seq[f].astype(np.int32))            # alpha 256: the descriptor itself
    col = [a['tmpl'][:, 0].astype(np.int64) for a in a1]
    assert col[0][5] == ref.SIM_MAX and col[1][5] == ref.SIM_MAX - 512 and col[2][5] == ref.SIM_MAX - 510
    steps = np.array([b - a for a, b in zip(col, col[1:])])
    want = np.array([256 * seq[f + 1].astype(np.int64) - col[f] for f in range(11)])
    assert ((steps == -1) & (want > -256)).any()                      # falls by less than a unit's worth: the floor
    assert ((steps == 0) & (want > 0)).any()
    assert not ((steps > 0) & (want < 256)).any()                     # and never rises by it
    _, outs, arrays = _proves(t['zero_refused'], gate=0)
    assert arrays[1]['has'][:2].tolist() == [1, 1] and not arrays[1]['tmpl'][:, 1].any() and outs[1]['sim'][:2] == [-1, -1]
    c = cases.retire_rebirth()
    _, outs, arrays = _proves(c)
    assert outs[1]['id'][0] == 2 and outs[1]['sim'][0] == -1 and outs[1]['count'] == 1 and outs[1]['missed'][0] == 0
    assert np.array_equal(arrays[1]['tmpl'][:, 0], 256 * cases.BLUE.astype(np.int32)) and arrays[1]['has'][0] == 1
    # the match did happen, and it is what retired the track: without the second detection the slot is empty after the frame
    alone = dict(c, frames=[c['frames'][0], cases._fr([((650.0, 200.0, 40.0, 60.0, 0.0), 0.9, 0)], 4)])
    _, o2, a2 = cases.restate(alone)
    assert o2[1]['count'] == 0 and not a2[1]['tmpl'].any() and not a2[1]['has'].any()


def test_branch_cases_descriptor_rows_are_settled():
    """Every row the GPU test compares with == has u == 0, and the named rows are what their names say."""
    frames = cases.frames()
    names = [n for n, _ in cases.bound_rows()]
    boxes = cases.bound_boxes()
    desc, info = ref.descriptors(frames, boxes)
    assert all(i is not None and i['u'] == 0 for row in info for i in row)
    for k, name in enumerate(names):
        for b, kk in ((0, k), (1, len(names) - 1 - k)):
            d = desc[b, kk].astype(np.int64)
            if name.startswith(('zero_size', 'at_')):
                assert d.sum() == 512 and sorted(d[d > 0].tolist()) == [256, 256] and (d[:64] > 0).sum() == 1, name
            elif name.startswith('past_'):
                assert d.sum() == 0, name
            else:
                assert d.sum() == 256 and d[:64].sum() == (0 if name == 'half_-y' else 128), (name, d.sum())       # half the taps count
    x, y = np.clip([cases.W, -1, 30, 30], 0, cases.W - 1), np.clip([20, 20, cases.H, -1], 0, cases.H - 1)
    for k, (xx, yy) in enumerate(zip(x, y)):                         # the border pixel the clamp picks
        px = frames[0, yy, xx].astype(np.int64)
        assert desc[0, 2 + k, (px[0] >> 6) * 16 + (px[1] >> 6) * 4 + (px[2] >> 6)] == 256, names[2 + k]
    assert float(np.float32(cases.up(cases.P29))) == cases.P29 + 64
    for name, fr in cases.edge_frames().items():
        _, info = ref.descriptors(fr, cases.edge_boxes())
        assert all(i is not None and i['u'] == 0 for row in info for i in row), name
        assert fr.shape[1:3] == {'h1': (1, cases.W), 'w1': (cases.H, 1), '1x1': (1, 1)}[name]
    one, _ = ref.descriptors(cases.edge_frames()['1x1'], cases.edge_boxes())
    assert all(np.array_equal(one[b, k], one[b, 0]) and one[b, k].sum() == 512 for b in range(2) for k in range(6))
    for k in (1, 2, 3, 5, 7):
        assert k % 4 and (k * 128 + 130) % 2 == 0
        d, info = ref.descriptors(cases.frames(2, 48, 66), cases.ragged_boxes(k))
        assert all(i['u'] == 0 for row in info for i in row) and (d.sum(axis=2) == 512).all()


def _header():
    return open(os.path.join(ROOT, 'include', 'mydet.h')).read()


def test_entry_points_are_declared_exported_and_bound():
    from mydetection_amd import _lib, ops
    header = _header()
    dll = ctypes.CDLL(_lib.LIB_PATH)
    for name, nargs in zip(NAMES, (10, 8, 24, 1)):
        assert re.search(r'\b(int|int64_t)\s+' + name + r'\s*\(', header)
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name]) == nargs
        assert hasattr(dll, name)
        assert getattr(_lib.lib(), name).argtypes == _lib.SIGNATURES[name]
    for name, value in (('MYDET_APPEAR_BINS', 128), ('MYDET_APPEAR_SAMPLES', 512), ('MYDET_APPEAR_SIM_MAX', 131072)):
        assert re.search(r'#define\s+' + name + r'\s+' + str(value) + r'\b', header)
        assert getattr(_lib, name[len('MYDET_'):]) == value
    assert 'typedef struct mydet_track_appear' in header
    assert re.search(r'#define\s+MYDET_ABI_VERSION\s+2\b', header) and _lib.ABI_VERSION == 2 and _lib.lib().mydet_abi_version() == 2
    s = _lib.TrackAppear
    assert ctypes.sizeof(s) == 32 and s.alpha.offset == 8 and s.reach.offset == 12 and s.update_thres.offset == 16
    for mt in (1, 63, 64, 512):
        assert _lib.lib().mydet_track_appear_state_words(mt) == ops.appear_state_words(mt) == (129 * mt + 3) // 4 * 4
    assert _lib.lib().mydet_track_appear_state_words(0) == 0 and _lib.lib().mydet_track_appear_state_words(513) == 0
    design = open(os.path.join(ROOT, 'DESIGN.md')).read()
    for text in ('sx = w * 0.75f / 16', '(i >> 4)*64 + (R >> 6)*16 + (G >> 6)*4 + (B >> 6)', 't += ((256*d - t) * alpha) >> 8'):
        assert text in header and text in design, text
    mk = open(os.path.join(ROOT, 'mydetection_amd', 'csrc', 'Makefile')).read()
    assert re.search(r'SRCS_EXACT\s*=.*\bappear\.hip\b', mk)


def test_abi_argument_checks_come_before_any_launch():
    """Every call below must fail its checks: the pointers are never dereferenced on the device."""
    from mydetection_amd import _lib
    lib = _lib.lib()
    null = ctypes.c_void_p(0)

    def good():
        l = _lib.DrawList()
        l.box, l.box_frame_stride, l.box_row_stride, l.K = 4096, 20, 4, 5
        return l

    def rgb(src=ctypes.c_void_p(4096), B=1, H=8, W=8, img=192, row=24, l=None, no_list=False, desc=8192, stride=640):
        return lib.mydet_appear_boxes_rgb_u8(src, B, H, W, img, row, null if no_list else ctypes.byref(l or good()), desc, stride, null)
    assert rgb(no_list=True) == -1 and rgb(src=null) == -1 and rgb(desc=None) == -1
    assert rgb(B=0) == -1 and rgb(H=0) == -1 and rgb(W=-1) == -1 and rgb(row=23) == -1 and rgb(img=-1) == -1
    assert rgb(desc=8194) == -1 and rgb(stride=639) == -1 and rgb(stride=641) == -1 and rgb(stride=-640) == -1
    assert rgb(B=65536) == -2 and rgb(H=(1 << 24) + 1) == -2
    for field, value in (('box', None), ('K', 0), ('K', 513), ('box_row_stride', -1), ('box_frame_stride', -1), ('angle_row_stride', -4),
                         ('count_stride', -1)):
        l = good()
        setattr(l, field, value)
        assert rgb(l=l) == -1, field

    def yuv(layout=_lib.YUV420_NV12, matrix=0, planes=(4096, 8192, None), rows=(8, 8, 0), src=True, desc=8192, stride=640):
        d = _lib.Yuv420Src()
        for i, p in enumerate(planes):
            d.plane[i], d.img_bytes[i], d.row_bytes[i] = p, 64, rows[i]
        d.layout, d.matrix = layout, matrix
        return lib.mydet_appear_boxes_yuv420(ctypes.byref(d) if src else null, 1, 8, 8, ctypes.byref(good()), desc, stride, null)
    assert yuv(src=False) == -1 and yuv(layout=7) == -1 and yuv(matrix=2) == -1 and yuv(planes=(4096, 8192, 12288)) == -1
    assert yuv(rows=(7, 8, 0)) == -1 and yuv(desc=None) == -1 and yuv(stride=638) == -1

    p, a, ap = _lib.TrackParams(), _lib.TrackAssoc(), _lib.TrackAppear()
    ap.alpha, ap.reach = 26, 2.0

    def track(ap=ap, a=a, mt=64, desc=1 << 20, astate=1 << 21, sim=1 << 22, how=1 << 23, no_ap=False, width=4):
        return lib.mydet_track_frames_appear_f32(4096, 4100, 4100, 1, 1, width, ctypes.byref(p), mt, 8192, 4096, 4096, 4096, 4096, 4096, 4096, 4096,
                                                 ctypes.byref(a), None, null if no_ap else ctypes.byref(ap), desc, astate, sim, how, null)
    assert track(no_ap=True) == -1 and track(desc=None) == -1 and track(astate=None) == -1 and track(sim=None) == -1 and track(how=None) == -1
    assert track(desc=(1 << 20) + 8) == -1 and track(astate=(1 << 21) + 4) == -1 and track(sim=(1 << 22) + 2) == -1 and track(width=3) == -1
    for field, value in (('gate', -1), ('gate', 131073), ('reid', -1), ('reid', 131073), ('alpha', 0), ('alpha', 257), ('reach', -1.0),
                         ('reach', float('inf')), ('reach', float('nan')), ('update_thres', float('nan'))):
        bad = _lib.TrackAppear()
        bad.alpha, bad.reach = 26, 2.0
        setattr(bad, field, value)
        assert track(ap=bad) == -1, (field, value)
    assert track(mt=513) == -2
    optimal = _lib.TrackAssoc()
    optimal.assign = _lib.TRACK_ASSIGN_OPTIMAL
    assert track(a=optimal) == -2                                    # MYDET_E_UNSUPP: the appearance runs with the greedy walk only


def test_ops_argument_rules_need_no_device():
    from mydetection_amd import _lib, ops
    for kw in (dict(gate=-0.1), dict(gate=1.5), dict(gate=float('nan')), dict(reid=2), dict(momentum=1.0), dict(momentum=-0.1),
               dict(momentum=0.9999), dict(reach=-1), dict(reach=float('inf')), dict(update_thres=float('nan'))):
        with pytest.raises(ValueError):
            ops.appear_set(**kw)
    with pytest.raises(ValueError):
        ops.appear_state_words(513)
    with pytest.raises(ValueError):
        ops.appear_state(0, 64, 'cpu')
    state = ops.appear_state(2, 64, 'cpu')
    assert state.shape == (2, 129 * 64) and state.dtype == torch.int32 and not state.any()
    v = ops.appear_state_views(state, 64)
    assert v['has'].shape == (2, 64) and v['tmpl'].shape == (2, 128, 64)
    v['tmpl'][1, 5, 7] = 9
    assert state[1, 64 + 5 * 64 + 7] == 9
    assert not ops.appear_reset_(state, 64).any()
    with pytest.raises(ValueError):
        ops.appear_state_views(state, 32)
    frames = torch.zeros((1, 8, 8, 3), dtype=torch.uint8)
    with pytest.raises(TypeError):
        ops.appear_boxes(frames.float(), torch.zeros((1, 2, 4)))
    with pytest.raises(TypeError):
        ops.appear_boxes(frames, torch.zeros((1, 2, 4), dtype=torch.float64))
    with pytest.raises(ValueError):
        ops.appear_boxes(frames, torch.zeros((2, 2, 4)))
    with pytest.raises(ValueError):
        ops.appear_boxes(frames, torch.zeros((1, 513, 4)))
    with pytest.raises(RuntimeError, match='no CPU path'):           # no fall-back on the host: a device tensor is required
        ops.appear_boxes(frames, torch.zeros((1, 2, 4)))
    par = ops.track_params((48, 64))
    rec = torch.zeros((1, _lib.REC_WORDS), dtype=torch.int32)
    tstate = torch.zeros((1, ops.track_state_words(64)), dtype=torch.int32)
    with pytest.raises(TypeError):
        ops.track_frames(rec, tstate, par, appear=(1, 2, 3))
    with pytest.raises(TypeError):
        ops.track_frames(rec, tstate, par, appear=ops.appear_set())
    with pytest.raises(ValueError):
        ops.track_frames(rec, tstate, par, assoc=ops.track_assoc('optimal'),
                         appear=(ops.appear_set(), torch.zeros((1, 512, 128), dtype=torch.uint16), ops.appear_state(1, 64, 'cpu')))


def test_api_argument_rules_need_no_device():
    from mydetection_amd.api import Appearance, Detector, Tracker
    a = Appearance()
    assert (a.gate, a.reid, a.momentum, a.reach, a.update_thres) == (0.3, 0.6, 0.9, 2.0, None) and a.state is None and a.last is None
    assert 'Appearance(gate=0.3' in repr(a)
    assert a.set(0.4).update_thres == np.float32(0.4) and Appearance(update_thres=0.7).set(0.4).update_thres == np.float32(0.7)
    for kw in (dict(gate=2), dict(reid=-1), dict(momentum=1), dict(reach=-2), dict(update_thres=float('nan'))):
        with pytest.raises(ValueError):
            Appearance(**kw)
    with pytest.raises(TypeError):
        Detector._pop_appearance({'appearance': 'yes'}, Tracker())
    with pytest.raises(ValueError):
        Detector._pop_appearance({'appearance': a}, None)
    with pytest.raises(ValueError):
        Detector._pop_appearance({'appearance': a}, Tracker(assign='optimal'))
    kwargs = {'appearance': a, 'conf_thres': 0.3}
    assert Detector._pop_appearance(kwargs, Tracker()) is a and kwargs == {'conf_thres': 0.3}
    assert Detector._pop_appearance({}, None) is None
    with pytest.raises(TypeError):
        Detector._no_tracker({'appearance': a}, 'frames_to_json')
    a.check_call(Tracker(streams=2, max_tracks=64), (48, 64))
    a.streams, a.max_tracks, a.img_hw = 2, 64, (48, 64)              # as bind() leaves them
    a.check_call(Tracker(streams=2, max_tracks=64), (48, 64))
    for tracker, hw in ((Tracker(streams=1, max_tracks=64), (48, 64)), (Tracker(streams=2, max_tracks=32), (48, 64)),
                        (Tracker(streams=2, max_tracks=64), (48, 66))):
        with pytest.raises(ValueError):
            a.check_call(tracker, hw)
    a.reset()                                                        # nothing bound: nothing to clear
