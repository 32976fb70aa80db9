"""GPU tests of zone and line counting (include/mydet.h: mydet_zones_frames; csrc/zones.hip).

The checker is tests/_zones_ref.py, a plain-Python restatement of the rule text that tests/test_zones_host.py holds to exact
fractions and to numbers derived by hand.  Every decision of the kernel is an integer comparison, so every output tensor,
every field of the state and the heat map equal the restatement with ==.  Synthetic tracker outputs (tests/_zones_cases.py)
everywhere; only the last test runs a model."""
import functools

import numpy as np
import pytest
import torch

import _zones_cases as zc
import _zones_ref as ref
from _arena import flat_arena

pytestmark = pytest.mark.gpu

OUTPUTS = ('inside', 'crossed', 'dwell', 'occupancy', 'zone_counts', 'line_counts')


@functools.lru_cache(maxsize=None)
def _cases():
    return {**zc.hand_cases(), **zc.fuzz_cases()}


@functools.lru_cache(maxsize=None)
def _expected(name):
    """The restatement's outputs, final state and heat map of a case in ONE call of all its frames: computed once, never changed."""
    case = _cases()[name]
    S, F, MT = case['out']['id'].shape
    zs = ref.ZoneSet(case['img_hw'], **case['zs'])
    streams = [ref.Stream(MT) for _ in range(S)]
    heat = None if zs.heat is None else np.zeros((S,) + tuple(zs.heat), np.int64)
    out = ref.run(zs, streams, case['out'], heat)
    return out, [st.arrays() for st in streams], heat


def _zone_set(case):
    from mydetection_amd import ops
    return ops.zone_set(case['img_hw'], **case['zs'])


def _on_device(out, lo=0, n=None):
    n = out['id'].shape[1] - lo if n is None else n
    return {k: torch.from_numpy(np.ascontiguousarray(v[:, lo:lo + n])).cuda() for k, v in out.items()}


def _assert_state(state, want, what):
    from mydetection_amd import ops
    got = {k: v.cpu().numpy() for k, v in ops.zones_state_views(state).items()}
    for s, arrays in enumerate(want):
        for k, v in arrays.items():
            assert np.array_equal(got[k][s], v), (what, 'state', k, s)


def _check(name, splits=None):
    """The kernel on a case, in one call or in the calls `splits` names, against the restatement's one call."""
    from mydetection_amd import ops
    case = _cases()[name]
    want, want_state, want_heat = _expected(name)
    S, F, MT = case['out']['id'].shape
    zs = _zone_set(case)
    state = ops.zones_state(S, MT, 'cuda')
    heat = ops.zones_heat(S, zs, 'cuda') if zs.heat_h else None
    parts, lo = [], 0
    for n in splits or [F]:
        parts.append(ops.zones_frames(_on_device(case['out'], lo, n), state, zs, heat=heat))
        lo += n
    assert lo == F
    for k in OUTPUTS:
        got = torch.cat([p[k] for p in parts], dim=1).cpu().numpy()
        assert got.dtype == np.int32 and got.shape == want[k].shape, (name, k, got.shape, want[k].shape)
        assert np.array_equal(got, want[k]), (name, k, np.argwhere(got != want[k])[:5].tolist())
    _assert_state(state, want_state, name)
    if heat is not None:
        assert np.array_equal(heat.cpu().numpy(), want_heat), name
    return parts


@pytest.mark.parametrize('name', sorted(zc.hand_cases()))
def test_hand_cases(name):
    """Lines met in every way (through A and B exactly, touched and continued, touched and returned, around the end, walked
    along), a track missed while it crosses (with and without coasting), slot reuse, a bad-class frame, the class filter,
    anchor='bottom', rotated boxes, non-finite boxes, heat cells at their boundaries: F = 7 (F = 1 for the heat cells), S = 1 or 3."""
    _check(name)
    exp = _cases()[name]['expect']
    if 'heat' in exp:                                                # the numbers derived by hand, straight on the device's
        assert np.array_equal(_expected(name)[2], exp['heat'])


@pytest.mark.parametrize('name', ['fuzz', 'fuzz_coasting_bottom', 'full', 'polygons_only', 'lines_only', 'mt1', 'mt512'])
def test_seeded_walks(name):
    """3 streams with different histories: 40 frames x 65 slots with births, deaths, reuse, misses, NaNs and bad-class frames on
    coordinates snapped to 1/32 pixel (also with coasting, anchor='bottom' and a class filter); 16 polygons of 16 vertices with
    16 lines, polygons only, lines only; max_tracks 1 and 512."""
    _check(name)


@pytest.mark.parametrize('name,splits', [('lines', [4, 3]), ('reuse', [4, 3]), ('bad_frame', [3, 4]), ('missed_coasting', [2, 5]),
                                         ('full', [4, 3]), ('mt1', [4, 3]), ('mt512', [4, 3]), ('mt512', [1] * 7), ('fuzz', [13, 27])])
def test_split_calls_equal_one_call(name, splits):
    """Two calls of F1 and F2 frames (and F calls of one frame) leave exactly the state, the outputs and the heat map of one call."""
    _check(name, splits)


def test_streams_are_independent_and_reset_restores():
    """Each stream of an S = 3 call equals an S = 1 call on its own frames; reset gives the fresh state back."""
    from mydetection_amd import ops
    case = _cases()['full']
    want, want_state, want_heat = _expected('full')
    S, F, MT = case['out']['id'].shape
    zs = _zone_set(case)
    for s in range(S):
        state = ops.zones_state(1, MT, 'cuda')
        heat = ops.zones_heat(1, zs, 'cuda')
        got = ops.zones_frames({k: torch.from_numpy(np.ascontiguousarray(v[s:s + 1])).cuda() for k, v in case['out'].items()}, state, zs, heat=heat)
        for k in OUTPUTS:
            assert np.array_equal(got[k].cpu().numpy(), want[k][s:s + 1]), (k, s)
        _assert_state(state, want_state[s:s + 1], f'stream {s}')
        assert np.array_equal(heat.cpu().numpy(), want_heat[s:s + 1])
    fresh = ops.zones_state(1, MT, 'cuda')
    assert not torch.equal(state, fresh) and int(fresh.abs().sum()) == 0
    ops.zones_reset_(state, MT)
    assert torch.equal(state, fresh)


def test_footprint_and_argument_checks():
    """Nothing outside the state, the heat map and the output buffers is written (guard bands around each, max_tracks = 65: no
    multiple of a wavefront) and every word of the outputs is; the wrong tensors are refused before a launch."""
    from mydetection_amd import _lib, ops
    case = _cases()['full']
    want, want_state, want_heat = _expected('full')
    S, F, MT = case['out']['id'].shape
    zs = _zone_set(case)
    Z, L = zs.n_polygons, zs.n_lines
    dev = torch.device('cuda')
    sw = ops.zones_state_words(MT)
    st_flat, chk_state = flat_arena(S * sw, dev)
    state = st_flat.view(torch.int32).view(S, sw)
    ops.zones_reset_(state, MT)
    torch.cuda.synchronize()
    assert chk_state.undefined_in_view() == (0, []) and int(state.abs().sum()) == 0
    chk_state.outside_untouched('state after reset')
    heat_flat, chk_heat = flat_arena(S * zs.heat_h * zs.heat_w, dev, fill='zero')
    heat = heat_flat.view(torch.int32).view(S, zs.heat_h, zs.heat_w)
    heat.zero_()
    shapes = {'inside': (S, F, MT), 'crossed': (S, F, MT), 'dwell': (S, F, MT, Z), 'occupancy': (S, F, Z), 'zone_counts': (S, F, Z, 4),
              'line_counts': (S, F, L, 2)}
    out, chks = {}, {}
    for k, shape in shapes.items():
        flat, chks[k] = flat_arena(int(np.prod(shape)), dev)
        out[k] = flat.view(torch.int32).view(shape)
    track_out = _on_device(case['out'])
    got = ops.zones_frames(track_out, state, zs, heat=heat, out=out)
    torch.cuda.synchronize()
    assert got is out
    chk_state.outside_untouched('state')
    chk_heat.outside_untouched('heat')
    for k, chk in chks.items():
        chk.outside_untouched(k)
        assert chk.undefined_in_view() == (0, []), k
        assert np.array_equal(out[k].cpu().numpy(), want[k]), k
    _assert_state(state, want_state, 'arena')
    assert np.array_equal(heat.cpu().numpy(), want_heat)
    # refused before a launch
    fresh = ops.zones_state(S, MT, dev)
    with pytest.raises(ValueError, match='heat'):
        ops.zones_frames(track_out, fresh, zs)                                   # the zone set has a heat grid
    with pytest.raises(ValueError, match='heat'):
        ops.zones_frames(track_out, fresh, zs, heat=torch.zeros(S, 3, 3, dtype=torch.int32, device=dev))
    with pytest.raises(ValueError, match='heat'):
        ops.zones_frames(track_out, fresh, ops.zone_set(case['img_hw'], lines=[zc.LINE]), heat=heat)
    with pytest.raises(ValueError, match='state'):
        ops.zones_frames(track_out, ops.zones_state(S, MT + 1, dev), zs, heat=heat)
    with pytest.raises(ValueError, match='streams'):
        ops.zones_frames(track_out, ops.zones_state(S + 1, MT, dev), zs, heat=heat)
    with pytest.raises(ValueError, match='missed'):
        ops.zones_frames(dict(track_out, missed=track_out['missed'].long()), fresh, zs, heat=heat)
    with pytest.raises(ValueError, match='dwell'):
        ops.zones_frames(track_out, fresh, zs, heat=heat, out=dict(out, dwell=out['dwell'][..., :1]))
    assert int(fresh.abs().sum()) == 0
    code = _lib.lib().mydet_zones_frames(*[ops._ptr(track_out[k]) for k in ('box', 'id', 'cls', 'missed', 'count')], S, F, MT,
                                         __import__('ctypes').byref(zs), fresh.data_ptr() + 4, ops._ptr(heat),
                                         *[ops._ptr(out[k]) for k in OUTPUTS], ops._stream())
    assert code == -1


# ---- model level ----

def _synthetic_frames(n, h, w, seed):
    from mydetection_amd import synth
    return np.stack([(synth.make_images(1, max(h, w), seed=seed + i)[0, :, :h, :w].permute(1, 2, 0).numpy() * 255).astype(np.uint8)
                     for i in range(n)])


def test_frame_methods_with_zones_equal_zones_frames_on_the_calls_tracks():
    """Detector('rapid').predict_frames(frames, tracker=, zones=) on 4 small synthetic frames: the objects are bit for bit those
    of the call without zones=, zones.last is ops.zones_frames on the same tracker output, the objects carry its bits, two calls
    continue the count, and the annotate / crop / NV12 forms take zones= too."""
    from mydetection_amd import ops, synth
    from mydetection_amd.api import Detector, Tracker, Zones
    from mydetection_amd.models.general import name_to_model
    m, cfg = name_to_model('rapid')
    m.load_state_dict(synth.make_state_dict(m.state_dict(), 'rapid'), strict=True)
    det = Detector(model_and_cfg=(m.eval().cuda(), cfg))
    H, W, B = 150, 200, 4
    kw = dict(input_size=128, conf_thres=0.001)
    tkw = dict(min_score=0.0005)                                                 # synthetic weights: keep the low scores alive
    base = _synthetic_frames(1, H, W, seed=90)[0]
    frames = np.stack([base, base, np.roll(base, 3, axis=1), np.roll(base, 6, axis=1)])
    # the two halves reach past the frame, so that every anchor of a live track is in one of them
    polygons = [[(-16, -16), (100, -16), (100, 166), (-16, 166)], [(100, -16), (216, -16), (216, 166), (100, 166)], [(40, 30), (160, 30), (100, 120)]]
    lines = [((100, 0), (100, 150)), ((0, 75), (200, 75))]
    zkw = dict(polygons=polygons, lines=lines, heat=(6, 8), names=['left', 'right', 'wedge', 'middle', 'waist'])

    with pytest.raises(ValueError, match='tracker='):
        det.predict_frames(frames, zones=Zones(**zkw), **kw)
    with pytest.raises(ValueError, match='bottom'):
        det.predict_frames(frames, tracker=Tracker(**tkw), zones=Zones(polygons=polygons, anchor='bottom'), **kw)   # a 'cxcywhd' model

    for streams, coasting in ((1, False), (2, True)):
        plain = det.predict_frames(frames, tracker=Tracker(streams=streams, **tkw), coasting=coasting, **kw)
        trk, zones = Tracker(streams=streams, **tkw), Zones(coasting=coasting, **zkw)
        got = det.predict_frames(frames, tracker=trk, coasting=coasting, zones=zones, **kw)
        # the same tracker output, and the zone launch on it
        (_, r), = det._frame_records(frames, _whole_records=True, **kw)
        tstate = ops.track_state(streams, 256, 'cuda')
        tout = ops.track_frames(r, tstate, ops.track_params((H, W), 'rotated', new_thres=kw['conf_thres'], **tkw))
        zs = ops.zone_set((H, W), polygons, lines, coasting=coasting, heat=(6, 8))
        zstate, zheat = ops.zones_state(streams, 256, 'cuda'), ops.zones_heat(streams, zs, 'cuda')
        zout = ops.zones_frames(tout, zstate, zs, heat=zheat)
        assert torch.equal(trk.state, tstate) and torch.equal(zones.state, zstate) and torch.equal(zones.heat, zheat)
        assert all(torch.equal(zones.last[k], zout[k]) for k in OUTPUTS)
        assert (zones.streams, zones.max_tracks, zones.img_hw) == (streams, 256, (H, W))
        total = 0
        for b, (o, p) in enumerate(zip(got, plain)):
            assert torch.equal(o.bboxes, p.bboxes) and torch.equal(o.scores, p.scores) and torch.equal(o.cats, p.cats) and torch.equal(o.obj_ids, p.obj_ids)
            assert p.zone_mask is None and p.line_events is None
            s, f = divmod(b, B // streams)
            keep = (tout['missed'][s, f] >= 0) if coasting else (tout['missed'][s, f] == 0)
            assert o.zone_mask.dtype == torch.int32 and torch.equal(o.zone_mask, zout['inside'][s, f][keep])
            assert torch.equal(o.line_events, zout['crossed'][s, f][keep])
            total += len(o)
        assert total > 0 and int(zout['zone_counts'][:, -1, :, 0].sum()) > 0 and int(zheat.sum()) > 0
        # every anchor is in the left or in the right half, never in both: the shared edge belongs to one of them
        seen = torch.cat([o.zone_mask for o in got])
        assert bool((((seen & 1) + ((seen >> 1) & 1)) == 1).all())
        # counts(): the state's numbers, by name
        counts = zones.counts()
        views = {k: v.cpu() for k, v in ops.zones_state_views(zstate).items()}
        assert len(counts) == streams and [c['frames'] for c in counts] == [B // streams] * streams
        for s, c in enumerate(counts):
            assert list(c['zones']) == ['left', 'right', 'wedge'] and list(c['lines']) == ['middle', 'waist']
            for z, name in enumerate(('left', 'right', 'wedge')):
                e = c['zones'][name]
                assert [e['entries'], e['exits'], e['lost'], e['visits']] == views['zone_counts'][s, z].tolist()
                assert e['occupancy'] == int(zout['occupancy'][s, -1, z]) and e['max_dwell'] == int(views['dwell_max'][s, z])
                assert e['mean_dwell'] == (int(views['dwell_sum'][s, z]) / e['visits'] if e['visits'] else None)
            for l, name in enumerate(('middle', 'waist')):
                assert [c['lines'][name]['pos'], c['lines'][name]['neg']] == views['line_counts'][s, l].tolist()
        if streams == 1:
            # a second call goes on counting: the frame counter and the cumulative rows continue
            det.predict_frames(frames, tracker=trk, zones=zones, **kw)
            more = ops.zones_frames(ops.track_frames(r, tstate, ops.track_params((H, W), 'rotated', new_thres=kw['conf_thres'], **tkw)), zstate, zs, heat=zheat)
            assert torch.equal(zones.state, zstate) and torch.equal(zones.heat, zheat) and all(torch.equal(zones.last[k], more[k]) for k in OUTPUTS)
            assert zones.counts()[0]['frames'] == 2 * B
            with pytest.raises(ValueError, match='bound to'):
                det.predict_frames(frames, tracker=Tracker(streams=2, **tkw), zones=zones, **kw)
            with pytest.raises(ValueError, match='bound to'):
                det.predict_frames(frames, tracker=Tracker(max_tracks=64, **tkw), zones=zones, **kw)
            assert torch.equal(zones.state, zstate)                              # refused before any launch
            zones.reset()
            trk.reset()
            assert int(zones.state.abs().sum()) == 0 and int(zones.heat.sum()) == 0 and zones.last is None
            again = det.predict_frames(frames, tracker=trk, zones=zones, **kw)
            assert all(torch.equal(a.zone_mask, g.zone_mask) and torch.equal(a.line_events, g.line_events) for a, g in zip(again, got))

    # the other frame methods take zones= through the same path
    want = [o.zone_mask for o in det.predict_frames(frames, tracker=Tracker(**tkw), zones=Zones(**zkw), **kw)]
    objs, drawn = det.annotate_frames(frames, tracker=Tracker(**tkw), zones=Zones(**zkw), **kw)
    assert all(torch.equal(o.zone_mask, w) for o, w in zip(objs, want)) and drawn.shape == (B, H, W, 3)
    objs, chips = det.crop_frames(frames, tracker=Tracker(**tkw), zones=Zones(**zkw), **kw)
    assert all(torch.equal(o.zone_mask, w) for o, w in zip(objs, want)) and len(chips) == B
    y = np.ascontiguousarray(frames[:, :, :, 0])
    uv = np.full((B, H // 2, W // 2, 2), 128, np.uint8)
    zones = Zones(**zkw)
    got = det.predict_frames_nv12(y, uv, tracker=Tracker(**tkw), zones=zones, **kw)
    ref_objs = det.predict_frames_nv12(y, uv, tracker=Tracker(**tkw), **kw)
    assert all(torch.equal(o.bboxes, p.bboxes) and torch.equal(o.obj_ids, p.obj_ids) and o.zone_mask is not None for o, p in zip(got, ref_objs))
    from mydetection_amd.api import Tiles
    zones = Zones(**zkw)
    got = det.predict_frames(frames, tiles=Tiles((96, 128), overlap=0.25), tracker=Tracker(**tkw), zones=zones, **kw)
    ref_objs = det.predict_frames(frames, tiles=Tiles((96, 128), overlap=0.25), tracker=Tracker(**tkw), **kw)
    assert all(torch.equal(o.bboxes, p.bboxes) and torch.equal(o.obj_ids, p.obj_ids) and len(o.zone_mask) == len(o) for o, p in zip(got, ref_objs))
    assert zones.counts()[0]['frames'] == B
    from mydetection_amd.api import Augment, Nms
    for extra in (dict(augment=Augment()), dict(nms=Nms(agnostic=True))):
        zones = Zones(**zkw)
        got = det.predict_frames(frames, tracker=Tracker(**tkw), zones=zones, **extra, **kw)
        ref_objs = det.predict_frames(frames, tracker=Tracker(**tkw), **extra, **kw)
        assert all(torch.equal(o.bboxes, p.bboxes) and torch.equal(o.obj_ids, p.obj_ids) and len(o.zone_mask) == len(o) for o, p in zip(got, ref_objs))
        assert zones.counts()[0]['frames'] == B and sum(len(o) for o in got) > 0
    with pytest.raises(TypeError):
        det.frames_to_json(frames, list(range(B)), zones=Zones(**zkw), **kw)
