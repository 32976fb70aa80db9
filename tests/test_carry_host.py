"""CPU tests of the key-frame carry: the settings and their errors, the C entry points and their argument checks, the binding rules
of KeyFrames, and the restatement tests/_carry_ref.py itself, held to the known motions of tests/_carry_cases.py (the GPU tests
hold the kernels to the restatement with ==)."""
import os
import re

import numpy as np
import pytest
import torch

import _carry_cases as cases
import _carry_ref as ref


def _meta_detector(name='yolov3_80'):
    from mydetection_amd.api import Detector
    from mydetection_amd.models.general import name_to_model
    with torch.device('meta'):
        m, cfg = name_to_model(name)
    return Detector(model_and_cfg=(m.eval(), cfg))


def _run_cases(rot=False):
    streams = [ref.Stream(), ref.Stream()]
    out = ref.run(streams, ref.luma_rgb(cases.rgb_frames()), cases.key_records(rot), 0, ref.Settings(**cases.SETTINGS), rot)
    return streams, out


def test_carry_set_range_checks_and_state_words():
    from mydetection_amd import _lib, ops
    c = ops.carry_set()
    assert (c.every, c.search, c.min_texture, c.max_diff) == (4, 8, 1024, 24)
    for bad in (dict(every=0), dict(every=17), dict(every=2.0), dict(every=True), dict(search=3), dict(search=17), dict(min_texture=-1),
                dict(min_texture=1 << 24), dict(max_diff=-1), dict(max_diff=256)):
        with pytest.raises(ValueError, match='carry_set'):
            ops.carry_set(**bad)
    assert ops.carry_set(every=1).every == 1 and ops.carry_set(every=16, search=16).search == 16
    assert ops.carry_state_words() == 512 * 336 == _lib.lib().mydet_carry_state_words() == ref.SLOTS * ref.SLOT_WORDS
    assert ref.Stream().words().shape == (ops.carry_state_words(),) and not ref.Stream().words().any()
    # the views of a host copy have the documented shapes
    v = ops.carry_state_views(torch.zeros(2, ops.carry_state_words(), dtype=torch.int32))
    assert {k: tuple(t.shape) for k, t in v.items()} == {
        'status': (2, 512), 'cell': (2, 512), 'cx16': (2, 512), 'cy16': (2, 512), 'offset': (2, 512, 2), 'rel': (2, 512, 2), 'box': (2, 512, 4),
        'angle': (2, 512), 'score': (2, 512), 'cls': (2, 512), 'coarse': (2, 512, 16, 16), 'patch': (2, 512, 32, 32)}
    with pytest.raises(ValueError, match='state'):
        ops.carry_state_views(torch.zeros(2, 100, dtype=torch.int32))
    with pytest.raises(RuntimeError):                                             # no CPU path
        ops.carry_state(1, 'cpu')
    # the key mask is one run of frames with a key frame every `every`
    assert ops.carry_first([True, False, False, True], 3) == 0 and ops.carry_first([False, True, False], 3) == 2
    assert ops.carry_first([False, False], 3) == 1 and ops.carry_first([True, True], 1) == 0
    for mask, every in (([True, True], 2), ([False, False, False], 3), ([True, False, True], 3), ([], 2), ([False], 1)):
        with pytest.raises(ValueError, match='key mask'):
            ops.carry_first(mask, every)


def test_entry_points_declared_exported_and_bound():
    from mydetection_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, 'include', 'mydet.h')).read()
    lib = _lib.lib()
    for name in ('mydet_carry_records_rgb_u8', 'mydet_carry_records_yuv420', 'mydet_carry_state_words', 'mydet_carry_reset'):
        assert re.search(r'\b' + name + r'\(', header), name
        assert name in _lib.SIGNATURES and getattr(lib, name).argtypes is not None
    assert 'carry.hip' in open(os.path.join(root, 'mydetection_amd', 'csrc', 'Makefile')).read()
    assert lib.mydet_abi_version() == 2
    for name, value in (('SLOTS', _lib.CARRY_SLOTS), ('SLOT_HEADER', _lib.CARRY_SLOT_HEADER), ('SLOT_WORDS', _lib.CARRY_SLOT_WORDS),
                        ('MAX_EVERY', _lib.CARRY_MAX_EVERY), ('HOW_NOT', _lib.CARRY_HOW_NOT), ('HOW_LEFT', _lib.CARRY_HOW_LEFT)):
        assert re.search(r'#define MYDET_CARRY_%s\s+%d\b' % (name, value), header), name


def test_c_argument_checks_refuse_before_any_launch():
    """Every call here has a null frame pointer at the least: a launch would fault, a refusal returns MYDET_E_BADARG."""
    import ctypes
    from mydetection_amd import _lib
    lib, null = _lib.lib(), None
    assert lib.mydet_carry_reset(null, 1, null) == -1 and lib.mydet_carry_reset(ctypes.c_void_p(16), 0, null) == -1
    assert lib.mydet_carry_reset(ctypes.c_void_p(8), 1, null) == -1                       # misaligned
    p = ctypes.c_void_p(4096)                                                             # never dereferenced: every call is refused
    good = _lib.CarrySet(3, 4, 1024, 24)

    def rgb(src=p, B=2, H=96, W=128, img=96 * 384, row=384, S=1, cset=good, first=0, key=p, stride=_lib.REC_WORDS, width=4, state=p,
            shift=null, ws=p, out=p, how=p, off=p, sad=p):
        return lib.mydet_carry_records_rgb_u8(src, B, H, W, img, row, S, None if cset is None else ctypes.byref(cset), first, key, stride, width,
                                              state, shift, ws, out, how, off, sad, null)
    for bad in (dict(src=null), dict(B=0), dict(S=0), dict(B=3, S=2), dict(S=65536, B=65536), dict(H=0), dict(W=0), dict(H=32769), dict(row=383),
                dict(img=-1), dict(cset=None), dict(cset=_lib.CarrySet(0, 4, 1024, 24)), dict(cset=_lib.CarrySet(17, 4, 1024, 24)),
                dict(cset=_lib.CarrySet(3, 3, 1024, 24)), dict(cset=_lib.CarrySet(3, 17, 1024, 24)), dict(cset=_lib.CarrySet(3, 4, -1, 24)),
                dict(cset=_lib.CarrySet(3, 4, 1024, 256)), dict(first=-1), dict(first=3), dict(width=3), dict(width=6), dict(key=null),
                dict(stride=_lib.REC_WORDS - 4), dict(stride=_lib.REC_WORDS + 1), dict(width=5), dict(state=null), dict(ws=null), dict(out=null),
                dict(how=null), dict(off=null), dict(sad=null), dict(state=ctypes.c_void_p(4100)), dict(out=ctypes.c_void_p(4100)),
                dict(key=ctypes.c_void_p(4100)), dict(how=ctypes.c_void_p(4098)), dict(shift=ctypes.c_void_p(4098))):
        assert rgb(**bad) == -1, bad
    src = _lib.Yuv420Src()
    assert lib.mydet_carry_records_yuv420(null, 2, 96, 128, 1, ctypes.byref(good), 0, p, _lib.REC_WORDS, 4, p, null, p, p, p, p, p, null) == -1
    assert lib.mydet_carry_records_yuv420(ctypes.byref(src), 2, 96, 128, 1, ctypes.byref(good), 0, p, _lib.REC_WORDS, 4, p, null, p, p, p, p, p, null) == -1
    src.plane[0], src.plane[1] = 4096, 8192
    src.row_bytes[0], src.row_bytes[1] = 128, 128
    src.img_bytes[0], src.img_bytes[1] = 96 * 128, 48 * 128
    for bad in (dict(S=0), dict(first=3), dict(state=null), dict(width=7)):
        kw = dict(S=1, first=0, state=p, width=4)
        kw.update(bad)
        assert lib.mydet_carry_records_yuv420(ctypes.byref(src), 2, 96, 128, kw['S'], ctypes.byref(good), kw['first'], p, _lib.REC_WORDS, kw['width'],
                                              kw['state'], null, p, p, p, p, p, null) == -1, bad


def test_keyframes_argument_and_binding_errors():
    from mydetection_amd import ops
    from mydetection_amd.api import KeyFrames, Tracker
    from mydetection_amd.api.bound import Bound
    from mydetection_amd.api.detection import Detector
    assert issubclass(KeyFrames, Bound) and Detector._COMPANIONS['keyframes'][0] is KeyFrames
    for bad in (dict(every=0), dict(every=17), dict(search=3), dict(search=17), dict(search=8.5), dict(min_texture=-1), dict(max_diff=300)):
        with pytest.raises(ValueError, match='carry_set'):
            KeyFrames(**bad)
    kf = KeyFrames()
    assert (kf.every, kf.search, kf.min_texture, kf.max_diff) == (4, 8, 1024, 24) and kf.state is None and kf.last is None
    # the key set of a call is host arithmetic on the counter, across calls of any length
    kf = KeyFrames(every=3)
    assert kf.key_mask(5) == [True, False, False, True, False]
    kf.frames = 5
    assert kf.key_mask(3) == [False, True, False] and ops.carry_first(kf.key_mask(3), 3) == 5 % 3
    kf.reset()
    assert kf.frames == 0 and kf.key_mask(1) == [True]

    det = _meta_detector()
    a = np.zeros((2, 96, 128, 3), np.uint8)
    y, uv = np.zeros((2, 96, 128), np.uint8), np.zeros((2, 48, 64, 2), np.uint8)
    for wrong in ('keyframes', True, 4):
        tracker = Tracker()
        with pytest.raises(TypeError, match='KeyFrames'):
            det.predict_frames(a, tracker=tracker, keyframes=wrong)
        assert tracker.state is None
    for call in (lambda **kw: det.predict_frames(a, **kw), lambda **kw: det.annotate_frames(a, **kw), lambda **kw: det.redact_frames(a, **kw),
                 lambda **kw: det.crop_frames(a, **kw), lambda **kw: det.predict_frames_nv12(y, uv, **kw)):
        with pytest.raises(ValueError, match='tracker='):
            call(keyframes=KeyFrames())
    bound = KeyFrames()
    bound.streams, bound.img_hw = 1, (48, 64)
    tracker = Tracker()
    with pytest.raises(ValueError, match='bound to'):
        det.predict_frames(a, tracker=tracker, keyframes=bound)
    assert tracker.state is None and tracker.img_hw is None
    with pytest.raises(TypeError, match='json'):
        det.frames_to_json(a, [0, 1], keyframes=KeyFrames())
    with pytest.raises(TypeError, match='json'):
        det.frames_nv12_to_json(y, uv, [0, 1], keyframes=KeyFrames())
    assert 'does NOT' in KeyFrames.__doc__


def test_restatement_gives_every_outcome_on_the_cases():
    streams, (rec, how, off, sad) = _run_cases()
    assert sorted(set(how.ravel().tolist())) == [ref.NONE, ref.KEY, ref.CARRIED, ref.FLAT, ref.LOST, ref.LEFT, ref.NOT]
    want = {'flat': [1, 3, 3, 1, 3, 3], 'nan': [1, 6, 6, 1, 6, 6], 'zero': [1, 6, 6, 1, 6, 6], 'painted': [1, 4, 4, 1, 2, 2],
            'leaver': [1, 2, 5, 0, 0, 0], 'small': [1, 2, 2, 1, 2, 2], 'mid': [1, 2, 2, 1, 2, 2], 'large': [1, 2, 2, 1, 2, 2], 'big': [1, 2, 2, 1, 2, 2]}
    for name, (s, j) in cases.SLOTS.items():
        assert how[s, :, j].tolist() == want[name], name
    # the cell sizes the named slots are there for: the state after the call holds the second key's slots
    cells = {name: streams[s].slots[j].s for name, (s, j) in cases.SLOTS.items()}
    assert (cells['small'], cells['mid'], cells['large'], cells['big']) == (1, 2, 3, 16)
    # counts: the alive slots, compacted; a key row is the key record itself
    assert rec[:, :, ref.REC_COUNT].tolist() == [[5, 2, 2, 5, 2, 2], [4, 3, 2, 3, 3, 3]]
    keys = cases.key_records()
    assert all((rec[s, f] == keys[s][k]).all() for s in range(2) for k, f in enumerate((0, 3)))
    assert rec[1, 2, ref.REC_INDEX:ref.REC_INDEX + 3].tolist() == [0, 1, 0]          # large, big; the rest zero
    # flat, lost and left report the SADs that decided them, once
    j = cases.SLOTS['painted'][1]
    assert sad[1, 1, j, 0] > 256 * cases.SETTINGS['max_diff'] and sad[1, 2, j].tolist() == [0, 0]
    j = cases.SLOTS['flat'][1]
    assert sad[0, 1, j, 1] - sad[0, 1, j, 0] < cases.SETTINGS['min_texture']


@pytest.mark.parametrize('rot', [False, True], ids=['plain', 'rotated'])
def test_restatement_follows_each_mover_exactly(rot):
    _, (rec, how, off, sad) = _run_cases(rot)
    scenes = cases.scenes()
    for name, step in cases.STEPS.items():
        s, j = cases.SLOTS[name]
        for f in range(cases.F):
            n = f % cases.EVERY
            if rot and name == 'mid' and n == 1:
                continue                     # rotated: side m / 2 gives s = 1, the 5-pixel step is beyond search * s = 4; found again at n = 2
            assert off[s, f, j].tolist() == [n * step[0], n * step[1]], (name, f)
            # the emitted box is the truth: key order is kept, so the mover's row is its slot
            box = rec[s, f, ref.REC_BBOX + 4 * j:ref.REC_BBOX + 4 * j + 4].view(np.float32)
            assert box.tolist() == [float(v) for v in scenes[s].box(name, f)], (name, f)
    if rot:
        assert rec[0, 1, ref.REC_ANGLE:ref.REC_ANGLE + 2].view(np.float32).tolist() == [0.0, 30.0]


def test_two_calls_equal_one_call_in_the_restatement():
    L, cfg, keys = ref.luma_rgb(cases.rgb_frames()), ref.Settings(**cases.SETTINGS), cases.key_records()
    whole, (rec, how, off, sad) = _run_cases()
    for cut in range(1, cases.F):
        streams = [ref.Stream(), ref.Stream()]
        k0 = sum(ref.key_mask(0, cases.EVERY, cut))
        a = ref.run(streams, L[:, :cut], [rows[:k0] for rows in keys], 0, cfg)
        b = ref.run(streams, L[:, cut:], [rows[k0:] for rows in keys], cut % cases.EVERY, cfg)
        for x, y, z in zip(a, b, (rec, how, off, sad)):
            assert (np.concatenate([x, y], axis=1) == z).all(), cut
        assert all((s.words() == w.words()).all() for s, w in zip(streams, whole)), cut


def test_box_conversion_and_tie_order():
    assert ref.to_fixed(10.03) == (True, 160) and ref.to_fixed(10.04) == (True, 161) and ref.to_fixed(-0.5) == (True, -8)
    assert ref.to_fixed(float('inf'))[0] is False and ref.to_fixed(float('nan'))[0] is False and ref.to_fixed(2.0 ** 26)[0] is False
    # equal SADs everywhere: the smallest motion, then the smaller dy, then the smaller dx
    flat = np.zeros((24, 24), np.int64)
    assert ref.search(np.zeros((16, 16), np.int64), flat, 4)[:2] == (0, 0)
    win = np.ones((18, 18), np.int64)
    win[0:16, 1:17] = 0                       # (dy, dx) = (-1, 0)
    win[1:17, 0:16] = 0                       # (0, -1): the same distance, the smaller dy wins
    assert ref.search(np.zeros((16, 16), np.int64), win, 1)[:3] == (-1, 0, 0)


def test_a_jump_is_followed_with_the_shift_and_lost_without_it():
    sc, frames, keys, shift = cases.jump_scene()
    L, cfg = ref.luma_rgb(frames), ref.Settings(**cases.SETTINGS)
    rec, how, off, _ = ref.run([ref.Stream()], L, keys, 0, cfg, shift=shift)
    assert how[0, :, 0].tolist() == [1, 2, 2] and off[0, 1:, 0].tolist() == [[13, -8], [14, -7]]
    for f in (1, 2):
        assert rec[0, f, ref.REC_BBOX:ref.REC_BBOX + 4].view(np.float32).tolist() == [float(v) for v in sc.box('small', f)]
    assert ref.run([ref.Stream()], L, keys, 0, cfg)[1][0, :, 0].tolist() == [1, 4, 4]


def _tracked_ids(records):
    """Per frame the ids of the tracks matched or born in it, by the tracker's restatement."""
    import _track_ref
    stream = _track_ref.Stream(16, _track_ref.Params(cases.HW))
    out = []
    for row in records:
        o = stream.step(*_track_ref.unpack_frame(row, 4))
        out.append(sorted(i for i, m in zip(o['id'], o['missed']) if m == 0))
    return out


def test_a_reversal_between_key_frames_keeps_its_id_only_with_the_carry():
    """The scene of the GPU test, tuned here: the carried records keep one id at the truth; the same key records with empty rows
    between them come back under a new id at the third key frame."""
    sc, frames, keys = cases.reversal_scene()
    rec, how, _, _ = ref.run([ref.Stream()], ref.luma_rgb(frames), keys, 0, ref.Settings(**cases.REVERSAL_SETTINGS))
    assert how[0, :, 0].tolist() == [1, 2, 2, 2, 1, 2, 2, 2, 1]
    for f in range(9):
        assert rec[0, f, ref.REC_BBOX:ref.REC_BBOX + 4].view(np.float32).tolist() == [float(v) for v in sc.box('turner', f)], f
    assert _tracked_ids(rec[0]) == [[1]] * 9
    sparse = np.zeros_like(rec[0])
    sparse[::4] = rec[0, ::4]
    ids = _tracked_ids(sparse)
    assert ids[0] == [1] and ids[4] == [1] and ids[8] == [2] and all(ids[f] == [] for f in (1, 2, 3, 5, 6, 7))
