"""GPU tests of tracking across video frames (include/mydet.h: mydet_track_frames_f32; csrc/track.hip).

The checker is tests/_track_ref.py.  In float32 it is the kernel's operation order, and the filter test holds the kernel's
state to it bit for bit after every frame of the sequences of tests/golden/kf_tracklet.npz -- the sequences on which
tests/test_track_host.py holds that restatement to the reference's KFTracklet.  The association cases are those of
tests/_track_cases.py: their decisions have margins (asserted on the float64 checker first), so the kernel's float32 IoUs
decide the same.  Synthetic records everywhere; only the last test runs a model."""
import numpy as np
import pytest
import torch

import _track_cases as tc
import _track_ref as ref
from _arena import flat_arena

pytestmark = pytest.mark.gpu

PLANES = ('x', 'v', 'pxx', 'pxv', 'pvv', 'score')


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def _params(img_hw, match, **kw):
    from mydetection_amd import ops
    return ops.track_params(img_hw, match, **kw)


def _state_np(state):
    from mydetection_amd import ops
    return {k: v.cpu().numpy() for k, v in ops.track_state_views(state).items()}


def _assert_state_equals(state, streams, what):
    """The device state of every stream against the float32 restatement, bit for bit."""
    got = _state_np(state)
    for s, stream in enumerate(streams):
        want = stream.arrays()
        for k in PLANES + ('cls', 'id', 'missed'):
            g, w = _bits(got[k][s]), _bits(want[k])
            assert np.array_equal(g, w), (what, 'stream', s, k, got[k][s], want[k])
        assert int(got['next_id'][s]) == stream.next_id and int(got['live'][s]) == sum(t is not None for t in stream.slots), (what, s)


def _track(rec, state, par):
    from mydetection_amd import ops
    out = ops.track_frames(torch.from_numpy(rec).cuda() if isinstance(rec, np.ndarray) else rec, state, par)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def test_filter_follows_the_float32_restatement_bit_for_bit(golden):
    """One detection per frame that always matches, over the fixture's sequences (one stream each, one launch per frame): after
    every frame the state views equal float32 _track_ref bit for bit, and the track lives exactly as long as the reference's
    is_feasible() says."""
    from mydetection_amd import ops
    g = golden('kf_tracklet')
    S, T, mt = len(g['names']), int(g['length'].max()), 4
    hw = tuple(int(v) for v in g['img_hw'])
    kw = dict(match_thres=0.3, new_thres=0.3, max_missed=1000)
    par = _params(hw, 'rotated', **kw)
    streams = [ref.Stream(mt, ref.Params(hw, np.float32, match='rotated', **kw)) for _ in range(S)]
    state = ops.track_state(S, mt, 'cuda')
    _assert_state_equals(state, streams, 'reset')
    cats = np.arange(S) % 3
    first_life = [True] * S
    for k in range(-1, T):
        frames = []
        for i in range(S):
            if k < 0:
                frames.append((g['init_box'][i][None], [g['init_score'][i]], [cats[i]]))
            elif k < g['length'][i] and g['has_z'][i, k]:
                frames.append((g['z'][i, k][None], [g['z_score'][i, k]], [cats[i]]))
            else:
                frames.append((np.zeros((0, 5), np.float32), [], []))
        rec = ref.pack_records(frames, 5)
        out = _track(rec, state, par)
        for i, stream in enumerate(streams):
            stream.step(*ref.unpack_frame(rec[i], 5))
        _assert_state_equals(state, streams, f'step {k}')
        for i in range(S):
            if 0 <= k < g['length'][i] and first_life[i]:
                alive = out['id'][i, 0, 0] == 1
                assert alive == bool(g['feasible'][i, k]), (g['names'][i], k)
                if alive:
                    assert out['missed'][i, 0, 0] == g['pred_count'][i, k] and out['cls'][i, 0, 0] == cats[i]
                    assert (out['missed'][i, 0, 0] == 0) == bool(g['has_z'][i, k])
                first_life[i] = alive
    assert first_life == [bool(g['feasible'][i, :g['length'][i]].all()) for i in range(S)] and not all(first_life) and any(first_life)


def _check_case(case, what):
    from mydetection_amd import ops
    hw, mt, width = tc.IMG_HW, case['max_tracks'], case['width']
    # the checker's side first: the decisions have margins, so float64 and the kernel's float32 IoUs decide alike
    chk = ref.Stream(mt, ref.Params(hw, np.float64, match=case['match'], **case['params']))
    f32 = ref.Stream(mt, ref.Params(hw, np.float32, match=case['match'], **case['params']))
    rec = ref.pack_records(case['frames'], width)
    want, boxes, scores = [], [], []
    for r in rec:
        want.append(chk.step(*ref.unpack_frame(r, width)))
        got32 = f32.step(*ref.unpack_frame(r, width))
        assert all(got32[k] == want[-1][k] for k in ('id', 'missed', 'count', 'dropped', 'match')), what
        a = f32.arrays()
        boxes.append(a['x'].T.copy())
        scores.append(a['score'].copy())
    assert chk.margins['iou_thres'] >= 0.05 and chk.margins['iou_gap'] >= 0.05 and chk.margins['score'] >= 1e-3, (what, chk.margins)
    assert chk.ties == case['ties'], what
    for w, e in zip(want, case['expect']):
        assert all(w[k] == e[k] for k in ('id', 'missed', 'count', 'dropped')), what
    # the kernel: every frame of the case in one launch
    state = ops.track_state(1, mt, 'cuda')
    out = _track(rec, state, _params(hw, case['match'], **case['params']))
    cls_of = {}
    for f, w in enumerate(want):
        assert out['id'][0, f].tolist() == w['id'], (what, f, out['id'][0, f], w['id'])
        assert out['missed'][0, f].tolist() == w['missed'], (what, f)
        assert int(out['count'][0, f]) == w['count'] and int(out['dropped'][0, f]) == w['dropped'], (what, f)
        if w['count'] < 0:
            assert not out['box'][0, f].any() and not out['score'][0, f].any() and not out['cls'][0, f].any()
            continue
        # the matched pairs: the filtered box and score of every slot are those of the restatement that took the checker's pairs
        assert np.array_equal(_bits(out['box'][0, f]), _bits(boxes[f])), (what, f, out['box'][0, f], boxes[f])
        assert np.array_equal(_bits(out['score'][0, f]), _bits(scores[f])), (what, f)
        b, s, c, n = ref.unpack_frame(rec[f], width)
        for slot, d in enumerate(w['match']):
            if d >= 0 and w['missed'][slot] == 0 and w['id'][slot] not in cls_of:
                cls_of[w['id'][slot]] = int(c[d])
        assert out['cls'][0, f].tolist() == [cls_of.get(i, 0) for i in w['id']], (what, f)
    _assert_state_equals(state, [f32], what)


@pytest.mark.parametrize('name', list(tc.cases()))
def test_association_cases(name):
    """Ids, classes, matched pairs and slot numbers of the hand-made cases, exactly."""
    _check_case(tc.cases()[name], name)


def test_association_at_the_full_512_detections_by_512_tracks():
    case = tc.full_case()
    assert case['max_tracks'] == 512 and all(len(f[1]) == 512 for f in case['frames'])
    _check_case(case, 'full')


def _scenario(S, F, seed):
    """S streams of F frames of rotated records: a few objects per stream that move, turn, appear and disappear, two classes."""
    rng = np.random.Generator(np.random.PCG64(seed))
    frames = []
    for s in range(S):
        n_obj = 5
        pos = np.stack([rng.uniform(80, 560, n_obj), rng.uniform(80, 400, n_obj), rng.uniform(40, 90, n_obj), rng.uniform(20, 50, n_obj),
                        rng.uniform(0, 180, n_obj)], axis=1)
        vel = np.stack([rng.uniform(-4, 4, n_obj), rng.uniform(-4, 4, n_obj), np.zeros(n_obj), np.zeros(n_obj), rng.uniform(-2, 2, n_obj)], axis=1)
        cats = rng.integers(0, 2, n_obj)
        for f in range(F):
            seen = [k for k in range(n_obj) if (k + f + s) % 5 > 1 and f >= k // 2]       # two-frame gaps: deaths and rebirths
            rng.shuffle(seen)
            b = (pos[seen] + vel[seen] * f + rng.uniform(-1, 1, (len(seen), 5))).astype(np.float32)
            frames.append((b.reshape(len(seen), 5), rng.uniform(0.35, 0.95, len(seen)).astype(np.float32), cats[seen]))
    return ref.pack_records(frames, 5)


def test_composition_reset_and_footprint():
    """F frames in one launch equal F launches of one frame and S = 2 equals two S = 1 trackers, bit for bit in state and
    outputs; strided records give the same; reset() restores the initial state; nothing outside the state and the output
    buffers is written (guard bands around each) and every word of them is."""
    from mydetection_amd import _lib, ops
    S, F, mt = 2, 6, 8
    dev = torch.device('cuda')
    rec = _scenario(S, F, seed=11)
    words = rec.shape[1]
    par = _params(tc.IMG_HW, 'rotated', max_missed=2)
    src = torch.from_numpy(rec).to(dev)
    sw = ops.track_state_words(mt)
    # one launch, in arenas
    st_flat, chk_state = flat_arena(S * sw, dev)
    state = st_flat.view(torch.int32).view(S, sw)
    fresh = ops.track_state(S, mt, dev)
    ops.track_reset_(state, mt)
    torch.cuda.synchronize()
    assert chk_state.undefined_in_view() == (0, []) and torch.equal(state, fresh)
    chk_state.outside_untouched('state after reset')
    shapes = {'box': (S, F, mt, 5), 'score': (S, F, mt), 'cls': (S, F, mt), 'id': (S, F, mt), 'missed': (S, F, mt), 'count': (S, F), 'dropped': (S, F)}
    dts = {'box': torch.float32, 'score': torch.float32, 'cls': torch.int64, 'id': torch.int64, 'missed': torch.int32, 'count': torch.int32,
           'dropped': torch.int32}
    out, chks = {}, {}
    for k, shape in shapes.items():
        n32 = int(np.prod(shape)) * (2 if dts[k] == torch.int64 else 1)
        flat, chks[k] = flat_arena(n32, dev)
        out[k] = flat.view(dts[k]).view(shape)
    ops.track_frames(src, state, par, out=out)
    torch.cuda.synchronize()
    chk_state.outside_untouched('state')
    for k, chk in chks.items():
        chk.outside_untouched(k)
        assert chk.undefined_in_view() == (0, []), k
    whole = {k: v.clone() for k, v in out.items()}
    whole_state = state.clone()
    assert int(whole['count'].max()) >= 3 and int((whole['missed'] > 0).sum()) > 0 and int(whole_state[:, 0].max()) > 6   # tracks, misses, deaths
    # F launches of one frame
    st1 = ops.track_state(S, mt, dev)
    v = src.view(S, F, words)
    for f in range(F):
        o = ops.track_frames(v[:, f:f + 1], st1, par)
        for k in shapes:
            assert torch.equal(o[k][:, 0], whole[k][:, f]), (k, f)
    assert torch.equal(st1, whole_state)
    # two S = 1 trackers
    for s in range(S):
        st = ops.track_state(1, mt, dev)
        o = ops.track_frames(src[s * F:(s + 1) * F], st, par)
        assert torch.equal(st[0], whole_state[s])
        for k in shapes:
            assert torch.equal(o[k][0], whole[k][s]), (k, s)
    # a frame-major buffer read through its strides, and a record dict
    fm = v.transpose(0, 1).contiguous()                                          # [F, S, words]
    st = ops.track_state(S, mt, dev)
    o = ops.track_frames(fm.transpose(0, 1), st, par)
    assert torch.equal(st, whole_state) and all(torch.equal(o[k], whole[k]) for k in shapes)
    st = ops.track_state(S, mt, dev)
    o = ops.track_frames(ops.record_views(src), st, par)
    assert torch.equal(st, whole_state) and all(torch.equal(o[k], whole[k]) for k in shapes)
    # reset
    ops.track_reset_(st, mt)
    assert torch.equal(st, fresh) and not torch.equal(whole_state, fresh)
    views = ops.track_state_views(st)
    assert views['next_id'].tolist() == [1] * S and not views['id'].any() and int(st.abs().sum()) == S
    # the C-level preconditions on device pointers: nothing is launched for a misaligned state
    lib = _lib.lib()
    code = lib.mydet_track_frames_f32(ops._ptr(src), F * words, words, S, F, 5, __import__('ctypes').byref(par), mt, st.data_ptr() + 4,
                                      *[ops._ptr(out[k]) for k in ('box', 'score', 'cls', 'id', 'missed', 'count', 'dropped')], ops._stream())
    assert code == -1


# ---- model level ----

def _synthetic_frames(n, h, w, seed):
    from mydetection_amd import synth
    return np.stack([(synth.make_images(1, max(h, w), seed=seed + i)[0, :, :h, :w].permute(1, 2, 0).numpy() * 255).astype(np.uint8)
                     for i in range(n)])


def test_predict_frames_with_a_tracker_equals_track_frames_on_the_calls_records():
    """Detector('rapid').predict_frames(frames, tracker=Tracker()) on 4 small synthetic frames: the objects are the tracks
    ops.track_frames gives on that call's own records (eager, then captured-graph replays); without tracker= nothing changes."""
    import PIL.Image
    from mydetection_amd import ops, synth
    from mydetection_amd.api import Detector, Tracker
    from mydetection_amd.models.general import name_to_model
    m, cfg = name_to_model('rapid')
    m.load_state_dict(synth.make_state_dict(m.state_dict(), 'rapid'), strict=True)
    det = Detector(model_and_cfg=(m.eval().cuda(), cfg))
    H, W, B = 150, 200, 4
    kw = dict(input_size=128, conf_thres=0.001)
    base = _synthetic_frames(1, H, W, seed=90)[0]
    frames = np.stack([base, base, np.roll(base, 3, axis=1), np.roll(base, 6, axis=1)])       # a still, then a slow pan
    tkw = dict(min_score=0.0005)                                                  # synthetic weights: keep the low scores alive
    # without tracker=: the records' own detections, the PIL path's bits, no ids
    plain = det.predict_frames(frames, **kw)
    (idxs, rec), = det._frame_records(frames, **kw)
    pil = det.predict_batch([PIL.Image.fromarray(f) for f in frames], **kw)
    counts = rec['count'].tolist()
    assert idxs == list(range(B)) and sum(counts) > 0
    for b, (o, p) in enumerate(zip(plain, pil)):
        k = counts[b]
        assert o.obj_ids is None and o.img_hw == (H, W) and len(o) == k
        assert torch.equal(o.bboxes, ops.record_boxes(rec, b, k)) and torch.equal(o.scores, rec['score'][b, :k]) and torch.equal(o.cats, rec['class_idx'][b, :k])
        assert torch.equal(o.bboxes, p.bboxes) and torch.equal(o.scores, p.scores) and torch.equal(o.cats, p.cats)

    def expected(streams, coasting, max_tracks=256):
        (_, r), = det._frame_records(frames, _whole_records=True, **kw)
        state = ops.track_state(streams, max_tracks, 'cuda')
        par = ops.track_params((H, W), 'rotated', new_thres=kw['conf_thres'], **tkw)
        out = ops.track_frames(r, state, par)
        objs = []
        for b in range(B):
            s, f = divmod(b, B // streams)
            missed = out['missed'][s, f]
            keep = (missed >= 0) if coasting else (missed == 0)
            objs.append((out['box'][s, f][keep], out['score'][s, f][keep], out['cls'][s, f][keep], out['id'][s, f][keep]))
        return objs, state, out

    total = 0
    for streams, coasting in ((1, False), (1, True), (2, False)):                 # eager first, then replays of the captured graph
        trk = Tracker(streams=streams, **tkw)
        got = det.predict_frames(torch.from_numpy(frames).cuda() if streams == 2 else frames, tracker=trk, coasting=coasting, **kw)
        want, state, out = expected(streams, coasting)
        assert trk.img_hw == (H, W) and trk.box_width == 5 and torch.equal(trk.state, state)
        assert len(got) == B
        for o, (bx, sc, cl, ids) in zip(got, want):
            assert o.img_hw == (H, W) and o.obj_ids.dtype == torch.int64 and o.bboxes.shape[1] == 5
            assert torch.equal(o.bboxes, bx) and torch.equal(o.scores, sc) and torch.equal(o.cats, cl) and torch.equal(o.obj_ids, ids)
            assert len(set(o.obj_ids.tolist())) == len(o)
            total += len(o)
        if streams == 1 and not coasting:
            ids0, ids1 = set(got[0].obj_ids.tolist()), set(got[1].obj_ids.tolist())
            assert ids0 and ids0 & ids1, 'no track continued from frame 0 to frame 1'
            # a second call continues the same tracks: the ids go on, none is used twice
            before = int(ops.track_state_views(trk.state)['next_id'][0])
            more = det.predict_frames(frames, tracker=trk, **kw)
            assert int(ops.track_state_views(trk.state)['next_id'][0]) >= before and len(more) == B
            trk.reset()
            assert torch.equal(trk.state, ops.track_state(1, 256, 'cuda')) and trk.img_hw == (H, W)
            again = det.predict_frames(frames, tracker=trk, **kw)
            assert all(torch.equal(a.obj_ids, g.obj_ids) and torch.equal(a.bboxes, g.bboxes) for a, g in zip(again, got))
            with pytest.raises(ValueError, match='one frame size'):
                det.predict_frames(frames[:, :100], tracker=trk, **kw)
    assert total > 0
    # the 4:2:0 form goes through the same code
    y = np.ascontiguousarray(frames[:, :, :, 0])
    uv = np.full((B, H // 2, W // 2, 2), 128, np.uint8)
    trk = Tracker()
    got = det.predict_frames_nv12(y, uv, tracker=trk, **kw)
    ref_objs = det.predict_frames_nv12(y, uv, **kw)
    assert len(got) == B and trk.img_hw == (H, W) and all(o.obj_ids is not None for o in got) and all(o.obj_ids is None for o in ref_objs)
    # and tiles= composes with tracker=
    from mydetection_amd.api import Tiles
    trk = Tracker()
    got = det.predict_frames(frames, tiles=Tiles((96, 128), overlap=0.25), tracker=trk, **kw)
    (_, r), = det._frame_records(frames, tiles=Tiles((96, 128), overlap=0.25), **kw)
    state = ops.track_state(1, 256, 'cuda')
    out = ops.track_frames(r, state, ops.track_params((H, W), 'rotated', new_thres=kw['conf_thres']))
    assert torch.equal(trk.state, state)
    for f, o in enumerate(got):
        keep = out['missed'][0, f] == 0
        assert torch.equal(o.obj_ids, out['id'][0, f][keep]) and torch.equal(o.bboxes, out['box'][0, f][keep])
