"""GPU tests of the counting overlay and of the trails launch (include/mydet.h: mydet_draw_overlay_rgb_u8, _yuv420_u8,
mydet_trails_frames; csrc/overlay.hip).

The checker is tests/_overlay_ref.py, a plain-Python restatement of the rule text that tests/test_overlay_host.py holds to exact
fractions.  Every decision of the kernels is an integer comparison, so the whole backing buffer of a painted target and every
output and state word of the trails equal the restatement with ==.  Synthetic counting outputs (tests/_overlay_cases.py)
everywhere; only the last test runs a model."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import _overlay_cases as oc
import _overlay_ref as ref
from _paint_targets import KINDS, Target, _dev

pytestmark = pytest.mark.gpu

SCENES = sorted(oc.scenes(*oc.RGB_HW))
TRAIL_OUTPUTS = ('points', 'len', 'bbox')


@functools.lru_cache(maxsize=None)
def _scene(name, hw):
    return oc.scenes(*hw)[name]


@functools.lru_cache(maxsize=None)
def _oplists(name, hw):
    """The restatement's operations of every frame of a scene: computed once, never changed."""
    sc = _scene(name, hw)
    return [ref.frame_ops(sc, o, *hw) for o in range(oc.B)]


def _style(scene):
    from mydetection_amd import ops
    return ops.draw_style(label_height=scene['label_height'], n_palette=scene['n_palette'])


def _inputs(scene, S):
    """The keyword arguments of ops.draw_overlay for a scene run as S streams of B / S frames."""
    from mydetection_amd import ops
    F = oc.B // S
    kw = dict(zones=scene['zones'], lines=scene['lines_on'], counters=scene['counters'], zone_alpha=scene['zone_alpha'],
              occupied_alpha=scene['occupied_alpha'])
    if scene['zones'] or scene['lines_on']:
        zs = ops.zone_set(scene['img_hw'], scene['pixels']['polygons'], scene['pixels']['lines'])
        Z, L = zs.n_polygons, zs.n_lines
        kw['geometry'] = ops.overlay_geometry(zs, scene['names'], scene['thickness'])
        kw['zones_out'] = {'occupancy': _dev(np.array(scene['occupancy'], np.int32).reshape(S, F, Z)),
                           'zone_counts': _dev(np.array(scene['zone_counts'], np.int32).reshape(S, F, Z, 4)),
                           'line_counts': _dev(np.array(scene['line_counts'], np.int32).reshape(S, F, L, 2))}
    tr = scene['trails']
    if tr is not None:
        MT, L = tr['points'].shape[1:3]
        kw['trails_out'] = {'points': _dev(tr['points'].reshape(S, F, MT, L, 2)), 'len': _dev(tr['len'].reshape(S, F, MT)),
                            'bbox': _dev(tr['bbox'].reshape(S, F, MT, 4))}
        kw['track_out'] = {'id': _dev(tr['id'].reshape(S, F, MT)), 'missed': _dev(tr['missed'].reshape(S, F, MT))}
        kw.update(trail_thickness=tr['thickness'], coasting=tr['coasting'])
    return kw


def _check_rgb(name, kind, S, seed=1):
    from mydetection_amd import ops
    hw = oc.RGB_HW
    scene = _scene(name, hw)
    tgt = Target(np.random.default_rng(seed), oc.B, hw[0], hw[1], 3, kind)
    before = tgt.back.copy()
    out = ops.draw_overlay(tgt.view, _style(scene), **_inputs(scene, S))
    torch.cuda.synchronize()
    assert out is tgt.view
    for b in range(oc.B):
        ref.paint_rgb(tgt.host[b], _oplists(name, hw)[b])
    tgt.check(f'{name} rgb {kind} S={S}')
    return before, tgt


def _check_yuv(name, layout, kind, S, matrix='bt601', full=False, seed=2):
    from mydetection_amd import ops
    hw = oc.YUV_HW
    H, W = hw
    H2, W2 = (H + 1) // 2, (W + 1) // 2
    planar = layout in ('i420', 'yv12')
    scene = _scene(name, hw)
    rng = np.random.default_rng(seed)
    ty = Target(rng, oc.B, H, W, 0, kind)
    tc = [Target(rng, oc.B, H2, W2, 0, kind) for _ in range(2)] if planar else [Target(rng, oc.B, H2, W2, 2, kind)]
    before = [t.back.copy() for t in [ty] + tc]
    planes = (ty.view,) + tuple(t.view for t in tc)
    out = ops.draw_overlay_yuv420(planes, layout, _style(scene), matrix=matrix, full_range=full, **_inputs(scene, S))
    torch.cuda.synchronize()
    assert out is planes
    for b in range(oc.B):
        if planar:
            u, v = (tc[0].host[b], tc[1].host[b]) if layout == 'i420' else (tc[1].host[b], tc[0].host[b])
        else:
            u, v = (tc[0].host[b, :, :, 0], tc[0].host[b, :, :, 1]) if layout == 'nv12' else (tc[0].host[b, :, :, 1], tc[0].host[b, :, :, 0])
        ref.paint_yuv(ty.host[b], u, v, _oplists(name, hw)[b], matrix, full)
    what = f'{name} {layout} {kind} S={S} {matrix} {full}'
    ty.check(what + ' Y')
    for t in tc:
        t.check(what + ' chroma')
    return before, [ty] + tc


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('name', SCENES)
def test_rgb_painter_equals_the_restatement(name, kind):
    """37 x 70 frames (full and partial 64 x 16 tiles both ways), B = 3 as S = 1 and as S = 3 streams, every byte of the backing
    buffer: a zone partly outside the frame, a vertex on a pixel centre, zones sharing an edge, overlapping zones (blend order),
    thickness 1, 2, 3 and 64, a line across tile borders, labels clamped at the right and the top edge and cut names, occupancy 0
    against > 0, multi-digit counters and one beyond 999999, trails of 2 and 32 points for 3, 64 and 65 slots, coasting tracks
    shown and not shown."""
    before, tgt = _check_rgb(name, kind, 1)
    _check_rgb(name, kind, 3)
    painted = not np.array_equal(before, tgt.back)
    assert painted == (name != 'nothing')                               # ... and a frame nothing reaches comes back byte-identical


@pytest.mark.parametrize('layout', ['nv12', 'nv21', 'i420', 'yv12'])
@pytest.mark.parametrize('name', SCENES)
def test_yuv420_painter_equals_the_restatement(name, layout):
    """35 x 131 planes (odd sizes, one full 128-wide tile and a partial one) of every 8-bit layout, the kind of target and the
    stream split cycling over the scenes; the same scenes as the RGB test, the chroma rule included."""
    k = SCENES.index(name) + ['nv12', 'nv21', 'i420', 'yv12'].index(layout)
    before, tgts = _check_yuv(name, layout, KINDS[k % 3], 1 if k % 2 else 3)
    painted = any(not np.array_equal(b, t.back) for b, t in zip(before, tgts))
    assert painted == (name != 'nothing')


def test_yuv420_every_kind_matrix_and_range():
    for kind in KINDS:
        _check_yuv('both', 'nv12', kind, 1, 'bt709', True)
        _check_yuv('both', 'i420', kind, 3, 'bt601', True)


def test_coasting_tracks_are_shown_only_with_coasting():
    """The two scenes differ in the coasting flag alone, and in pixels: a track with missed > 0 has a trail in one of them."""
    hw = oc.RGB_HW
    a = np.zeros(hw + (3,), np.uint8)
    b = a.copy()
    ref.paint_rgb(a, _oplists('both', hw)[0])
    ref.paint_rgb(b, _oplists('both_no_coasting', hw)[0])
    assert not np.array_equal(a, b)


# ------------------------------------------------------------------------------------------------------------------ trails
@functools.lru_cache(maxsize=None)
def _trail_expected(name):
    case = oc.trail_cases()[name]
    S, F, MT = case['out']['id'].shape
    ts = case['ts']
    streams = [ref.TrailStream(MT, ts['max_points'], ts.get('anchor', 'center'), ts.get('classes')) for _ in range(S)]
    return ref.run_trails(streams, case['out']), [st.arrays() for st in streams]


def _on_device(out, lo=0, n=None, streams=None):
    n = out['id'].shape[1] - lo if n is None else n
    sel = slice(None) if streams is None else streams
    return {k: torch.from_numpy(np.ascontiguousarray(v[sel, lo:lo + n])).cuda() for k, v in out.items()}


def _assert_trail_state(state, MT, L, want, what):
    from mydetection_amd import ops
    got = {k: v.cpu().numpy() for k, v in ops.trails_state_views(state, MT, L).items()}
    for s, arrays in enumerate(want):
        for k, v in arrays.items():
            assert np.array_equal(got[k][s], v), (what, 'state', k, s)


def _check_trails(name, splits=None):
    from mydetection_amd import ops
    case = oc.trail_cases()[name]
    want, want_state = _trail_expected(name)
    S, F, MT = case['out']['id'].shape
    ts = ops.trail_set(**case['ts'])
    state = ops.trails_state(S, MT, ts.max_points, 'cuda')
    parts, lo = [], 0
    for n in splits or [F]:
        parts.append(ops.trails_frames(_on_device(case['out'], lo, n), state, ts))
        lo += n
    assert lo == F
    for k in TRAIL_OUTPUTS:
        got = torch.cat([p[k] for p in parts], dim=1).cpu().numpy()
        assert got.dtype == np.int32 and got.shape == want[k].shape, (name, k, got.shape, want[k].shape)
        assert np.array_equal(got, want[k]), (name, k, np.argwhere(got != want[k])[:5].tolist())
    _assert_trail_state(state, MT, ts.max_points, want_state, name)
    return state


@pytest.mark.parametrize('name', sorted(oc.trail_cases()))
def test_trails_equal_the_restatement(name):
    """State and all three outputs, in one call and in two: ring wrap, slot reuse, a bad-class frame, a non-finite anchor, the
    class filter, anchor='bottom', 1 .. 512 slots, S = 1 and 3."""
    _check_trails(name)
    F = oc.trail_cases()[name]['out']['id'].shape[1]
    _check_trails(name, [F // 2, F - F // 2])
    _check_trails(name, [1] * 3 + [F - 3])


def test_trail_streams_are_independent_and_reset_restores():
    from mydetection_amd import ops
    name = 'fuzz_L7'
    case = oc.trail_cases()[name]
    want, want_state = _trail_expected(name)
    S, F, MT = case['out']['id'].shape
    ts = ops.trail_set(**case['ts'])
    one = ops.trails_state(1, MT, 7, 'cuda')
    got = ops.trails_frames(_on_device(case['out'], streams=slice(1, 2)), one, ts)
    for k in TRAIL_OUTPUTS:
        assert np.array_equal(got[k].cpu().numpy()[0], want[k][1]), k
    _assert_trail_state(one, MT, 7, want_state[1:2], 'stream 1 alone')
    fresh = ops.trails_state(1, MT, 7, 'cuda')
    assert int(fresh.abs().sum()) == 0 and int(one.abs().sum()) > 0
    assert ops.trails_reset_(one, MT, 7) is one and torch.equal(one, fresh)
    again = ops.trails_frames(_on_device(case['out'], streams=slice(1, 2)), one, ts)
    assert all(torch.equal(again[k], got[k]) for k in TRAIL_OUTPUTS)


# --------------------------------------------------------------------------------------------------------- argument checks
def test_refused_arguments_launch_nothing():
    """MYDET_E_BADARG / MYDET_E_UNSUPP of the entry points with real device buffers: the code, and every buffer unchanged."""
    from mydetection_amd import _lib, ops
    h = _lib.lib()
    case = oc.trail_cases()['reuse_L2']
    out = _on_device(case['out'])
    S, F, MT = out['id'].shape
    ts = ops.trail_set(2)
    state = ops.trails_state(S, MT, 2, 'cuda')
    res = {k: torch.full(shape, 7, dtype=torch.int32, device='cuda') for k, shape in
           (('points', (S, F, MT, 2, 2)), ('len', (S, F, MT)), ('bbox', (S, F, MT, 4)))}
    keep = {k: v.clone() for k, v in res.items()}
    p = lambda t: ctypes.c_void_p(t.data_ptr())                          # noqa: E731

    def trails(S_=S, F_=F, MT_=MT, ts_=ts, state_=state, len_=res['len']):
        return h.mydet_trails_frames(p(out['box']), p(out['id']), p(out['cls']), p(out['missed']), p(out['count']), S_, F_, MT_,
                                     ctypes.byref(ts_) if ts_ is not None else None, p(state_) if state_ is not None else None,
                                     p(res['points']), p(len_) if len_ is not None else None, p(res['bbox']), None)
    bad_l, bad_anchor, bad_cls = ops.trail_set(2), ops.trail_set(2), ops.trail_set(2)
    bad_l.max_points, bad_anchor.anchor, bad_cls.n_classes = 33, 2, 17
    assert trails(S_=0) == -1 and trails(F_=0) == -1 and trails(MT_=0) == -1 and trails(ts_=None) == -1 and trails(state_=None) == -1
    assert trails(len_=None) == -1 and trails(ts_=bad_l) == -1 and trails(ts_=bad_anchor) == -1 and trails(ts_=bad_cls) == -1
    assert trails(MT_=513) == -2
    assert h.mydet_trails_state_words(513, 2) == 0 and h.mydet_trails_state_words(4, 1) == 0 and h.mydet_trails_state_words(4, 33) == 0
    assert h.mydet_trails_state_words(3, 2) == ops.trails_state_words(3, 2) == 24
    assert h.mydet_trails_reset(None, 1, 4, 2, None) == -1 and h.mydet_trails_reset(p(state), 1, 4, 1, None) == -1
    assert h.mydet_trails_reset(p(state), 1, 513, 2, None) == -2
    torch.cuda.synchronize()
    assert all(torch.equal(res[k], keep[k]) for k in res) and int(state.abs().sum()) == 0

    # the painter
    hw = oc.RGB_HW
    scene = _scene('both', hw)
    frames = torch.full((oc.B,) + hw + (3,), 9, dtype=torch.uint8, device='cuda')
    kw = _inputs(scene, 1)
    o, tensors = ops._overlay_struct('test', oc.B, **kw)
    buf = kw['geometry'].buffer('cuda')
    o.geometry = p(buf)
    st, keep_style = _style(scene).struct('cuda')
    atlas = ops.glyph_atlas(8, 'cuda')
    st.atlas, st.ch, st.cw = p(atlas), atlas.shape[1], atlas.shape[2]

    def paint(o_=o, st_=st, B_=oc.B, H_=hw[0], W_=hw[1], row_=hw[1] * 3):
        return h.mydet_draw_overlay_rgb_u8(p(frames), B_, H_, W_, hw[0] * hw[1] * 3, row_, ctypes.byref(o_) if o_ is not None else None,
                                           ctypes.byref(st_) if st_ is not None else None, None)

    def changed(**fields):
        c = _lib.Overlay.from_buffer_copy(o)
        for k, v in fields.items():
            setattr(c, k, v)
        return c
    assert paint(o_=None) == -1 and paint(st_=None) == -1 and paint(B_=0) == -1 and paint(H_=0) == -1 and paint(W_=32769) == -1
    assert paint(B_=2) == -1 and paint(row_=hw[1] * 3 - 1) == -1
    for fields in (dict(flags=0), dict(flags=8), dict(counters=8), dict(zone_alpha=256), dict(occupied_alpha=-1), dict(thickness=0),
                   dict(thickness=65), dict(trail_thickness=0), dict(n_polygons=17), dict(n_lines=-1), dict(coasting=2), dict(geometry=None),
                   dict(occupancy=None), dict(zone_counts=None), dict(line_counts=None), dict(trail_points=None), dict(trail_len=None),
                   dict(trail_bbox=None), dict(id=None), dict(missed=None), dict(max_tracks=0), dict(max_points=1), dict(max_points=33),
                   dict(S=2)):
        assert paint(o_=changed(**fields)) == -1, fields
    assert paint(o_=changed(max_tracks=513)) == -2
    no_atlas = _lib.DrawStyle.from_buffer_copy(st)
    no_atlas.atlas = None
    no_palette = _lib.DrawStyle.from_buffer_copy(st)
    no_palette.palette = None
    small = _lib.DrawStyle.from_buffer_copy(st)
    small.ch = 7
    assert paint(st_=no_atlas) == -1 and paint(st_=no_palette) == -1 and paint(st_=small) == -1
    # a 10-bit layout, through the C entry point and through ops
    y16, uv16 = torch.zeros((oc.B, 8, 8), dtype=torch.int16, device='cuda'), torch.zeros((oc.B, 4, 4, 2), dtype=torch.int16, device='cuda')
    src = _lib.Yuv420Src()
    src.plane[0], src.plane[1], src.layout = y16.data_ptr(), uv16.data_ptr(), _lib.YUV420_P010
    src.img_bytes[0], src.img_bytes[1], src.row_bytes[0], src.row_bytes[1] = 128, 64, 16, 16
    assert h.mydet_draw_overlay_yuv420_u8(ctypes.byref(src), oc.B, 8, 8, ctypes.byref(o), ctypes.byref(st), None) == -1
    with pytest.raises(ValueError, match='p010'):
        ops.draw_overlay_yuv420((y16, uv16), 'p010', _style(scene), **kw)
    torch.cuda.synchronize()
    assert bool((frames == 9).all()) and int(y16.abs().sum()) == 0
    del tensors, keep_style


# ------------------------------------------------------------------------------------------------------- through the detector
def test_annotate_frames_with_overlay_equals_the_ops_on_the_calls_outputs():
    """Detector('rapid').annotate_frames(frames, tracker=, zones=, overlay=) on 4 small synthetic frames, twice: the objects are bit
    for bit those of the call without overlay=, `drawn` is ops.draw_overlay followed by ops.draw_boxes on the call's own tracker,
    zones and trails outputs, for RGB and NV12, and the second call continues trails and counters."""
    from mydetection_amd import ops, synth
    from mydetection_amd.api import Detector, Draw, Overlay, Tracker, Zones
    from mydetection_amd.models.general import name_to_model
    from mydetection_amd.utils.visualization import objects_to_rows
    m, cfg = name_to_model('rapid')
    m.load_state_dict(synth.make_state_dict(m.state_dict(), 'rapid'), strict=True)
    det = Detector(model_and_cfg=(m.eval().cuda(), cfg))
    H, W, B = 150, 200, 4
    kw = dict(input_size=128, conf_thres=0.001)
    tkw = dict(min_score=0.0005)
    base = np.random.default_rng(90).integers(0, 256, size=(H, W, 3), dtype=np.uint8)
    frames = np.stack([base, base, np.roll(base, 3, axis=1), np.roll(base, 6, axis=1)])
    polygons = [[(-16, -16), (100, -16), (100, 166), (-16, 166)], [(100, -16), (216, -16), (216, 166), (100, 166)], [(40, 30), (160, 30), (100, 120)]]
    lines = [((100, 0), (100, 150)), ((0, 75), (200, 75))]
    zkw = dict(polygons=polygons, lines=lines, names=['left', 'right', 'wedge', 'middle', 'waist'])
    okw = dict(counters=('occupancy', 'entries', 'visits'), trails=3, thickness=2, trail_thickness=1, label_height=10)
    draw = Draw(thickness=1, labels=('class', 'id'), label_height=10)

    with pytest.raises(ValueError, match='tracker='):
        det.annotate_frames(frames, overlay=Overlay(**okw), **kw)
    with pytest.raises(ValueError, match='zones='):
        det.annotate_frames(frames, tracker=Tracker(**tkw), overlay=Overlay(**okw), **kw)
    with pytest.raises(TypeError, match='Overlay'):
        det.annotate_frames(frames, tracker=Tracker(**tkw), overlay='yes', **kw)
    with pytest.raises(TypeError, match='annotate_frames'):
        det.predict_frames(frames, tracker=Tracker(**tkw), zones=Zones(**zkw), overlay=Overlay(**okw), **kw)
    with pytest.raises(ValueError, match='p010'):
        det.annotate_frames_yuv((np.zeros((B, 8, 8), np.uint16), np.zeros((B, 4, 4, 2), np.uint16)), 'p010', tracker=Tracker(**tkw),
                                zones=Zones(**zkw), overlay=Overlay(**okw), **kw)

    for streams, coasting in ((1, False), (2, True)):
        plain_trk, plain_zones = Tracker(streams=streams, **tkw), Zones(coasting=coasting, **zkw)
        trk, zones, overlay = Tracker(streams=streams, **tkw), Zones(coasting=coasting, **zkw), Overlay(**okw)
        total = 0
        for call in range(2):
            src = np.roll(frames, 5 * call, axis=2)
            plain, plain_drawn = det.annotate_frames(torch.from_numpy(src).cuda(), draw=draw, tracker=plain_trk, coasting=coasting, zones=plain_zones, **kw)
            got, drawn = det.annotate_frames(torch.from_numpy(src).cuda(), draw=draw, tracker=trk, coasting=coasting, zones=zones, overlay=overlay, **kw)
            for o, p in zip(got, plain):
                assert torch.equal(o.bboxes, p.bboxes) and torch.equal(o.scores, p.scores) and torch.equal(o.cats, p.cats)
                assert torch.equal(o.obj_ids, p.obj_ids) and torch.equal(o.zone_mask, p.zone_mask) and torch.equal(o.line_events, p.line_events)
                total += len(o)
            assert torch.equal(trk.state, plain_trk.state) and torch.equal(zones.state, plain_zones.state)
            # the overlay launch and the box launch on the call's own outputs
            want = torch.from_numpy(src).cuda()
            geo = ops.overlay_geometry(ops.zone_set((H, W), polygons, lines, coasting=coasting), zkw['names'], 2)
            style = ops.draw_style(label_height=10)
            ops.draw_overlay(want, style, geometry=geo, zones_out=zones.last, trails_out=overlay.last, track_out=overlay._track_out,
                             counters=okw['counters'], trail_thickness=1, coasting=coasting)
            assert not torch.equal(want, torch.from_numpy(src).cuda())
            boxes, counts, scores, classes, ids = objects_to_rows(got, 'cuda')
            ops.draw_boxes(want, boxes, draw.style((H, W), True), counts=counts, scores=scores, classes=classes, ids=ids)
            assert torch.equal(drawn, want) and not torch.equal(drawn, plain_drawn)
            if call == 1:                                                # trails and counters went on: frames seen, ring fills
                assert int(ops.zones_state_views(zones.state)['now'][0]) == 2 * B // streams
                fill = ops.trails_state_views(overlay.state, 256, 3)['fill']
                assert int(fill.max()) == 3
        assert total > 0 and (overlay.streams, overlay.max_tracks, overlay.img_hw) == (streams, 256, (H, W))
        # NV12: the same call on planes, against the ops on the call's outputs
        y = torch.from_numpy(np.ascontiguousarray(frames[..., 1])).cuda()
        uv = torch.from_numpy(np.ascontiguousarray(frames[:, ::2, ::2, :2])).cuda()
        trk, zones, overlay = Tracker(streams=streams, **tkw), Zones(coasting=coasting, **zkw), Overlay(**okw)
        y0, uv0 = y.clone(), uv.clone()
        got, drawn = det.annotate_frames_nv12(y, uv, draw=draw, tracker=trk, coasting=coasting, zones=zones, overlay=overlay, **kw)
        ops.draw_overlay_yuv420((y0, uv0), 'nv12', ops.draw_style(label_height=10), geometry=geo, zones_out=zones.last, trails_out=overlay.last,
                                track_out=overlay._track_out, counters=okw['counters'], trail_thickness=1, coasting=coasting)
        boxes, counts, scores, classes, ids = objects_to_rows(got, 'cuda')
        ops.draw_boxes_yuv420((y0, uv0), 'nv12', boxes, draw.style((H, W), True), counts=counts, scores=scores, classes=classes, ids=ids)
        assert torch.equal(drawn[0], y0) and torch.equal(drawn[1], uv0)
        # another shape is refused, and reset() forgets the trails
        with pytest.raises(ValueError, match='bound to'):
            det.annotate_frames(frames[:, :100], tracker=Tracker(streams=streams, **tkw), zones=Zones(**zkw), overlay=overlay, **kw)
        overlay.reset()
        assert int(overlay.state.abs().sum()) == 0 and overlay.last is None
