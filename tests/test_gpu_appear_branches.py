"""GPU tests of the branches tests/test_gpu_appear.py leaves alone: every tracker comparison is == against the plain-Python
restatement (tests/_appear_ref.py) on every per-frame output, the tracker state and the appearance state
(test_gpu_appear._assert_equals_restatement), every descriptor comparison goes through test_gpu_appear._check_desc.  The cases are
tables and builders in tests/_appear_cases.py; tests/test_appear_host.py proves on the restatement alone that each is what this
table takes it for (the outcome occurs, the margins hold, the rule altered gives other outputs).  Outputs are passed in filled
with a pattern, the records are a strided view, both states sit inside guard words, and the guards, the padding words of the
states, the records and the descriptors are checked after every run.  tk = csrc/track.hip, ap = csrc/appear.hip.

test_streams_and_slot_counts     three streams with a scene each, in one launch and in two: s * astate_words, (s F + f) * 512 * 128,
      o * MT + tid (tk:201, tk:296, tk:568); all six <BW, ROT, MODE, true> instances at MT = 65 -- blockDim 128, slot_ok false in
      the second wave, a template stride that is odd, three padding words in the appearance state (tk:694) --, one instance each
      at MT = 1, 63, 100, 130; at MT = 1 every second object is dropped
test_many_detections             150 detections a frame: s_bmask words 0 .. 2 (tk:416, tk:426), three re-identifications in one frame
      with winners in three waves and s_red[rc & 1] over four candidates (tk:439), and at MT = 64 the p0 += nthr ballot loops
      (tk:411, tk:513), 87 candidates, born < nbirth (tk:534)
test_levels_at_equality          S == gate passes in the high band (how 1) and in the low one (how 2), S == reid passes; one more
      does not (tk:378, tk:435)
test_gate_changes_the_outcome    the best IoU gated out and the second track takes the detection in that step; every track refuses
      and the detection is born; the walk refuses and the re-identification takes (tk:378 -> tk:429)
test_reid_guards                 missed >= 2, the class, new_thres, the high band: one changed at a time (tk:413-414, tk:429)
test_reach                       <= at equality and one float32 step beyond, each argument of the max deciding, y alone, reach 0, the
      shifted prediction (tk:430-433, tk:273)
test_template_arithmetic         alpha 1 and 256, a bin of 512, a row of zeros, the state after every frame (tk:486); the zero row
      refused by the gate
test_retire_and_rebirth_in_one_frame   tk:505 then tk:554 on one column in one frame
test_ragged_k                    K % 4 != 0: the k < K guard of the last group (ap:75), a frame stride of K * 128 + 130 (ap:76)
test_edge_frames, test_the_bound H = 1, W = 1, 1 x 1; zero-size boxes; taps on, beyond and across 2^29 (ap:66-67)
"""
import numpy as np
import pytest
import torch

import _appear_cases as cases
import _appear_ref as ref
import _track_ref
import _yuv420_ref
from test_gpu_appear import BANDS, SENTINEL, STATE_KEYS, VARIANTS, _assert_equals_restatement, _bits, _check_desc, _dev

pytestmark = pytest.mark.gpu

FILL = 0x5a5a5a5a
PAD = 64                                                             # guard words on either side of a state
OUTS = dict(box=(5, torch.float32), score=(0, torch.float32), cls=(0, torch.int64), id=(0, torch.int64), missed=(0, torch.int32),
            sim=(0, torch.int32), how=(0, torch.int32))


def _arena(S, words):
    arena = torch.full((PAD + S * words + PAD,), FILL, dtype=torch.int32, device='cuda')
    return arena, arena[PAD:PAD + S * words].view(S, words)


def _filled(S, n, mt):
    out = {k: torch.empty((S, n, mt) + ((last,) if last else ()), dtype=dt, device='cuda') for k, (last, dt) in OUTS.items()}
    out.update(count=torch.empty((S, n), dtype=torch.int32, device='cuda'), dropped=torch.empty((S, n), dtype=torch.int32, device='cuda'))
    for t in out.values():
        t.view(torch.uint8).fill_(0x5a)
    return out


def _run(streams, width, mt, match='iou', params=None, appear=None, assoc=None, shifts=None, cuts=None):
    """streams [(frames, descs)] of one length F through ops.track_frames on fresh states, in calls of `cuts` frames, the
    appearance settings as raw integers on the struct.  Returns (outs: per stream the dict of [F, ...] arrays, snaps: after every
    call, per stream (tracker state views, appearance state views)), all numpy."""
    from mydetection_amd import _lib, ops
    S, F = len(streams), len(streams[0][0])
    host = np.stack([_track_ref.pack_records(fr, width) for fr, _ in streams])
    words = host.shape[2]
    big = torch.full((S, F + 1, words + 8), FILL, dtype=torch.int32, device='cuda')
    rec = big[:, :F, :words]
    rec.copy_(_dev(host))
    assert rec.stride(0) > F * rec.stride(1) > F * words
    desc = _dev(np.stack([ds for _, ds in streams]))
    held = [(big, big.clone()), (desc, desc.clone())]
    par = ops.track_params(cases.TRACK_HW, match, **(params or {}))
    tas = ops.track_assoc(**assoc) if assoc else None
    a = dict(dict(gate=0, reid=0, alpha=26, reach=2.0, update_thres=0.3), **(appear or {}))
    aset = ops.appear_set(None, None, 0.9, a['reach'], a['update_thres'])
    aset.gate, aset.reid, aset.alpha = a['gate'], a['reid'], a['alpha']
    sw, aw = ops.track_state_words(mt), ops.appear_state_words(mt)
    sarena, state = _arena(S, sw)
    aarena, astate = _arena(S, aw)
    ops.track_reset_(state, mt)
    astate.zero_()
    sh = None if shifts is None else _dev(np.stack(shifts).astype(np.int32))
    parts, snaps, lo = [], [], 0
    for n in (cuts or [F]):
        out = _filled(S, n, mt)
        got = ops.track_frames(rec[:, lo:lo + n], state, par, max_tracks=mt, out=out, assoc=tas,
                               shift=None if sh is None else sh[:, lo:lo + n].contiguous(),
                               appear=(aset, desc[:, lo:lo + n].contiguous(), astate))
        assert got is out
        parts.append(out)
        tv = {k: v.cpu().numpy() for k, v in ops.track_state_views(state, mt).items()}
        av = {k: v.cpu().numpy() for k, v in ops.appear_state_views(astate, mt).items()}
        snaps.append([({k: v[s] for k, v in tv.items()}, {k: v[s] for k, v in av.items()}) for s in range(S)])
        lo += n
    assert lo == F
    for arena in (sarena, aarena):                                   # the words around the states
        assert bool((arena[:PAD] == FILL).all()) and bool((arena[-PAD:] == FILL).all())
    # the padding words inside them: three at MT = 65 for the appearance state
    assert not astate[:, (1 + _lib.APPEAR_BINS) * mt:].any() and not state[:, _lib.TRACK_STATE_HEADER + _lib.TRACK_SLOT_WORDS * mt:].any()
    assert all(torch.equal(t, before) for t, before in held)         # the records with their gaps, the descriptors
    outs = [{k: torch.cat([p[k] for p in parts], dim=1)[s].cpu().numpy() for k in parts[0]} for s in range(S)]
    return outs, snaps


_RESTATED = {}


def _restated(key, c):
    """The case's restatement, computed once."""
    if key not in _RESTATED:
        _RESTATED[key] = cases.restate(c)
    return _RESTATED[key]


def _hold(key, c, cuts=None):
    """One case on the device == its restatement, and the outcomes it is for; with `cuts` the state after every call too."""
    stream, outs, arrays = _restated(key, c)
    got, snaps = _run([(c['frames'], c['descs'])], c['width'], c['mt'], c['match'], c['params'], c['appear'], c['assoc'],
                      None if c['shifts'] is None else [c['shifts']], cuts)
    out = got[0]
    _assert_equals_restatement(out, snaps[-1][0][0], snaps[-1][0][1], stream, outs, arrays, key)
    lo = 0
    for n, snap in zip(cuts or [], snaps):
        lo += n
        _assert_state(snap[0], arrays[lo - 1], (key, lo))
    for f, k, h in c['expect']:
        assert out['how'][f, k] == h, (key, f, k, h, out['how'][f].tolist())
    return out, snaps, outs, arrays


def _assert_state(snap, want, what):
    tv, av = snap
    for k in STATE_KEYS:
        assert np.array_equal(_bits(tv[k]), _bits(want[k])), (what, k)
    assert np.array_equal(av['has'], want['has']) and np.array_equal(av['tmpl'], want['tmpl']), what


# ---- streams and slot counts ----

SLOTS = [(v, b, 65) for v in sorted(VARIANTS) for b in (False, True)] + [('bw4', False, 1), ('bw5', True, 63), ('rot', False, 100), ('rot', True, 130)]


@pytest.mark.parametrize('variant,bands,mt', SLOTS)
def test_streams_and_slot_counts(variant, bands, mt):
    v = VARIANTS[variant]
    scenes = cases.stream_scenes(v['width'], low=bands, rot=variant != 'bw4')
    F = len(scenes[0][0])
    appear = dict(gate=ref.level(0.3), reid=ref.level(0.5), alpha=ref.alpha_of(0.8), reach=2.0, update_thres=0.5)
    assoc = BANDS if bands else None
    want = [ref.run(fr, ds, v['width'], cases.TRACK_HW, mt, params=dict(match=v['match']), appear=appear, assoc=assoc) for fr, ds in scenes]
    for cuts in (None, [4, F - 4]):
        got, snaps = _run(scenes, v['width'], mt, v['match'], appear=appear, assoc=assoc, cuts=cuts)
        for s, (stream, outs, arrays) in enumerate(want):          # every stream its own single-stream restatement
            _assert_equals_restatement(got[s], snaps[-1][s][0], snaps[-1][s][1], stream, outs, arrays, (variant, bands, mt, cuts, s))
        if cuts:
            for s in range(3):
                _assert_state(snaps[0][s], want[s][2][3], (variant, bands, mt, 'after 4 frames', s))
    hows = [{int(h) for h in g['how'].reshape(-1)} for g in got]
    if mt >= 63:
        assert hows[0] >= {-1, 0, 1, 3, 4} | ({2} if bands else set()) and 3 in hows[1] and int(got[2]['id'].max()) == 2
    else:                                                            # one slot: the second object is dropped in every frame
        busy = [f for f, fr in enumerate(scenes[0][0]) if fr is not None and len(fr[1]) >= 2]
        assert len(busy) == 6 and (got[0]['dropped'][busy] >= 1).all() and (got[2]['dropped'][:4] == 1).all() and not got[1]['dropped'].any()


# ---- many detections ----

@pytest.mark.parametrize('mt', (192, 64))
def test_many_detections(mt):
    c = cases.many(mt)
    out, snaps, outs, arrays = _hold(('many', mt), c, cuts=[1, 5])
    f = cases.MANY_FRAME
    if mt == 192:
        assert [int(out['id'][f, k]) for k in cases.MANY_LOST] == [k + 1 for k in cases.MANY_LOST]          # the tracks' own ids
        assert (out['how'][f] == 3).sum() == 3 and (out['how'][f] == 4).sum() == 3 and not out['dropped'].any()
        assert out['missed'][f, cases.MANY_STRANGER] == 3 and out['id'][f, 150:153].tolist() == [151, 152, 153]
    else:
        assert (out['dropped'] > 0).all() and out['dropped'][0] == cases.MANY_N - 64 and (out['how'][0] == 4).all()
        assert np.array_equal(snaps[0][0][1]['tmpl'].T, 256 * c['descs'][0][:64].astype(np.int32))            # born: the descriptors
        assert (out['how'][f] == 3).sum() == 1 and out['id'][f, 3] == 4


# ---- integer levels, the gate, the guards, the reach ----

@pytest.mark.parametrize('name', sorted(cases.threshold_cases()))
def test_levels_at_equality(name):
    c = cases.threshold_cases()[name]
    out, _, _, _ = _hold(('level', name), c)
    assert (out['sim'][len(c['frames']) - 1, 0] == 65536) == name.endswith('65536')


@pytest.mark.parametrize('name', sorted(cases.gate_cases()))
def test_gate_changes_the_outcome(name):
    out, _, _, _ = _hold(('gate', name), cases.gate_cases()[name])
    if name == 'walk_refuses_reid_takes':
        assert out['sim'][4, 0] == 65536 and out['id'][4, 0] == 1 and out['missed'][3, 0] == 2


@pytest.mark.parametrize('name', sorted(cases.guard_cases()))
def test_reid_guards(name):
    c = cases.guard_cases()[name]
    out, _, _, _ = _hold(('guard', name), c)
    assert (3 in out['how'][-1]) == name.endswith('base')


@pytest.mark.parametrize('name', sorted(cases.reach_cases()))
def test_reach(name):
    c = cases.reach_cases()[name]
    out, _, _, _ = _hold(('reach', name), c)
    assert out['box'][3, 0, :2].tolist() == [200.0, 200.0]          # the track stood still: the prediction is exact
    assert (out['how'][4, 0] == 3) == name.endswith('_at') and (out['how'][4, 1] == 4) == name.endswith('_past')


# ---- templates ----

@pytest.mark.parametrize('name', sorted(cases.template_cases()))
def test_template_arithmetic(name):
    c = cases.template_cases()[name]
    out, snaps, outs, arrays = _hold(('template', name), c, cuts=[1] * len(c['frames']))          # the state after every frame
    if name == 'alpha_256':
        for f, d in enumerate(cases.TEMPLATE_SEQ):
            assert np.array_equal(snaps[f][0][1]['tmpl'][:, 0], 256 * d.astype(np.int32)), f
    if name == 'zero_refused':
        assert out['sim'][1, :2].tolist() == [-1, -1] and not snaps[1][0][1]['tmpl'][:, 1].any() and snaps[1][0][1]['has'][:2].tolist() == [1, 1]


def test_retire_and_rebirth_in_one_frame():
    c = cases.retire_rebirth()
    out, snaps, _, _ = _hold(('retire', 0), c)
    av = snaps[-1][0][1]
    assert out['how'][1, 0] == 4 and out['sim'][1, 0] == -1 and out['id'][1, 0] == 2 and out['count'][1] == 1
    assert np.array_equal(av['tmpl'][:, 0], 256 * cases.BLUE.astype(np.int32)) and av['has'][0] == 1 and not av['tmpl'][:, 1:].any()


# ---- descriptor ----

def _desc_view(B, K, stride):
    """uint16 [B, K, 128] with `stride` elements between frames, inside a sentinel arena."""
    arena = torch.full((4096 + (B - 1) * stride + K * 128 + 4096,), SENTINEL, dtype=torch.uint16, device='cuda')
    return arena, arena.as_strided((B, K, 128), (stride, 128, 1), 4096)


def _desc_rows(arena, B, K, stride):
    """The rows of the view as numpy [B, K, 128]; everything else of the arena must be the sentinel still."""
    host = arena.cpu().numpy().copy()
    rows = []
    for b in range(B):
        lo = 4096 + b * stride
        rows.append(host[lo:lo + K * 128].reshape(K, 128).copy())
        host[lo:lo + K * 128] = SENTINEL
    assert (host == SENTINEL).all(), np.flatnonzero(host != SENTINEL)[:8]
    return np.stack(rows)


@pytest.mark.parametrize('source', ('rgb', 'i010'))
def test_ragged_k(source):
    from mydetection_amd import ops
    if source == 'rgb':
        frames = cases.frames(2, 48, 66)
        image = _dev(frames)
    else:
        host = _yuv420_ref.random_planes(source, 2, 48, 66, seed=17)
        image = tuple(torch.from_numpy(p.view(np.int16)).cuda() for p in host)
        frames = _yuv420_ref.to_rgb(host, source, 'bt709', True)
    for K in (1, 2, 3, 5, 7):
        boxes, counts = cases.ragged_boxes(K), np.array([K, K - 1], np.int32)
        stride = K * 128 + 130
        arena, out = _desc_view(2, K, stride)
        if source == 'rgb':
            got = ops.appear_boxes(image, _dev(boxes), counts=_dev(counts), out=out)
        else:
            got = ops.appear_boxes_yuv420(image, source, _dev(boxes), counts=_dev(counts), out=out, matrix='bt709', full_range=True)
        assert got.data_ptr() == out.data_ptr() and out.stride(0) == stride
        rows = _desc_rows(arena, 2, K, stride)
        exact, loose = _check_desc(rows, frames, boxes, counts, (source, K))
        assert (exact, loose) == (2 * K - 1, 0) and not rows[1, K - 1].any() and (rows[0].sum(axis=1) == 512).all()


def test_edge_frames():
    from mydetection_amd import ops
    boxes = cases.edge_boxes()
    for name, frames in cases.edge_frames().items():
        got = ops.appear_boxes(_dev(frames), _dev(boxes)).cpu().numpy()
        assert _check_desc(got, frames, boxes, None, name) == (12, 0) and (got.sum(axis=2) == 512).all()
        if name == '1x1':                                            # every row is that pixel, whatever the box
            assert all(np.array_equal(got[b, k], got[b, 0]) and np.count_nonzero(got[b, k]) == 2 for b in range(2) for k in range(6))


def test_the_bound():
    from mydetection_amd import ops
    frames, boxes = cases.frames(), cases.bound_boxes()
    names = [n for n, _ in cases.bound_rows()]
    K = len(names)
    arena, out = _desc_view(2, K, K * 128 + 2)
    ops.appear_boxes(_dev(frames), _dev(boxes), out=out)
    got = _desc_rows(arena, 2, K, K * 128 + 2)
    assert _check_desc(got, frames, boxes, None, 'bound') == (2 * K, 0)
    for k, name in enumerate(names):
        for row in (got[0, k], got[1, K - 1 - k]):
            total = 512 if name.startswith(('zero_size', 'at_')) else 0 if name.startswith('past_') else 256
            assert row.sum() == total and (total != 512 or sorted(row[row > 0].tolist()) == [256, 256]), name
