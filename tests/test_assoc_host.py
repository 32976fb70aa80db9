"""CPU tests of the tracker's association modes (include/mydet.h: mydet_track_assoc, mydet_track_frames_assoc_f32): the numpy
restatement tests/_assoc_ref.py against brute force and against tests/_track_ref.py, the argument errors of api.Tracker and
ops.track_assoc, and the C ABI (declared, exported, bound, constants, struct layout, argument checks before any launch)."""
import ctypes
import os
import re

import numpy as np
import pytest

import _assoc_ref as aref
import _mot_ref
import _track_cases as tc
import _track_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _random_problem(rng, n, mt):
    iou = np.round(rng.uniform(0.0, 1.0, (n, mt)), 3)
    ok = (iou > 0.3) & (rng.uniform(size=(n, mt)) < 0.8)             # under the threshold, or ineligible for another reason
    return iou, ok


def test_optimal_total_equals_brute_force_on_random_matrices():
    """200 problems of up to 6 detections x 6 tracks (plus a dummy column per row): the restatement's total is the least over
    all one-to-one assignments, and no ineligible pair comes back."""
    rng = np.random.Generator(np.random.PCG64(2024))
    sizes = [(6, 6), (6, 3), (3, 6), (1, 1), (1, 6), (6, 1)]
    while len(sizes) < 200:
        sizes.append((int(rng.integers(1, 6)), int(rng.integers(1, 7))))
    matched = unmatched_rows = 0
    for n, mt in sizes:
        iou, ok = _random_problem(rng, n, mt)
        cost = aref.cost_matrix(iou, ok)
        assert cost.shape == (n, mt + n) and (cost[:, mt:] == 65536).all()
        assert ((cost[:, :mt] == 131072) == ~ok).all() and (cost[:, :mt][ok] == 65536 - np.floor(iou[ok] * 65536)).all()
        pairs, total = aref.optimal_pairs(cost, mt)
        assert total == _mot_ref.brute_force(cost), (n, mt)
        assert len(set(r for r, _ in pairs)) == len(pairs) == len(set(c for _, c in pairs))
        for r, c in pairs:
            assert ok[r, c] and iou[r, c] > 0.3
        assert total == sum(int(cost[r, c]) for r, c in pairs) + 65536 * (n - len(pairs))
        gap, ties, unchecked = aref.optimal_gap(cost, mt, pairs)
        assert unchecked == 0 and gap > 0
        matched += len(pairs)
        unmatched_rows += n - len(pairs)
    assert matched > 200 and unmatched_rows > 50


def test_optimal_keeps_both_identities_where_greedy_loses_one():
    """The example of the rules: A 0.60 / 0.50 to tracks 1 / 2, B 0.55 to track 1 only."""
    iou = np.array([[0.60, 0.50], [0.55, 0.0]])
    cost = aref.cost_matrix(iou, iou > 0.3)
    pairs, total = aref.optimal_pairs(cost, 2)
    assert pairs == [(0, 1), (1, 0)] and total == 2 * 65536 - int(np.floor(0.5 * 65536)) - int(np.floor(0.55 * 65536))
    gap, ties, _ = aref.optimal_gap(cost, 2, pairs)
    assert ties == 0 and gap == int(np.floor(0.5 * 65536)) + int(np.floor(0.55 * 65536)) - int(np.floor(0.6 * 65536))


def test_exact_tie_takes_the_lower_column():
    iou = np.array([[0.5, 0.5]])
    cost = aref.cost_matrix(iou, iou > 0.3)
    pairs, _ = aref.optimal_pairs(cost, 2)
    assert pairs == [(0, 0)] and aref.optimal_gap(cost, 2, pairs)[:2] == (np.inf, 1)


@pytest.mark.parametrize('name', list(tc.cases()) + ['full'])
def test_greedy_without_bands_is_the_tracker_of_old(name):
    case = tc.full_case() if name == 'full' else tc.cases()[name]
    for dtype in (np.float64, np.float32) if name != 'full' else (np.float64,):
        par = ref.Params(tc.IMG_HW, dtype, match=case['match'], **case['params'])
        old, new = ref.Stream(case['max_tracks'], par), aref.Stream(case['max_tracks'], par)
        for r in ref.pack_records(case['frames'], case['width']):
            frame = ref.unpack_frame(r, case['width'])
            assert new.step(*frame) == old.step(*frame)
        a, b = old.arrays(), new.arrays()
        assert all(np.array_equal(a[k], b[k]) for k in a) and old.next_id == new.next_id and old.ties == new.ties


def test_tracker_and_track_assoc_argument_errors():
    from mydetection_amd import _lib, ops
    from mydetection_amd.api import Tracker
    t = Tracker()
    assert (t.assign, t.low_thres, t.high_thres, t.low_match_thres) == ('greedy', None, None, None) and t.assoc(0.3) is None
    assert "assign='greedy'" in repr(t) and 'low_thres=None' in repr(t)
    a = Tracker(assign='optimal').assoc(0.3)
    assert isinstance(a, _lib.TrackAssoc) and (a.assign, a.bands) == (_lib.TRACK_ASSIGN_OPTIMAL, 0)
    t = Tracker(assign='optimal', low_thres=0.1, match_thres=0.4)
    a = t.assoc(0.3)
    assert (a.assign, a.bands, a.high_thres, a.low_thres, a.low_match_thres) == (1, 1, np.float32(0.3), np.float32(0.1), np.float32(0.4))
    assert "assign='optimal'" in repr(t) and 'low_thres=0.1' in repr(t) and 'high_thres=None' in repr(t) and 'low_match_thres=None' in repr(t)
    a = Tracker(low_thres=0.1, high_thres=0.6, low_match_thres=0.5).assoc(0.3)
    assert (a.assign, a.bands, a.high_thres, a.low_match_thres) == (0, 1, np.float32(0.6), np.float32(0.5))
    with pytest.raises(ValueError, match='low_thres < high_thres'):
        t.assoc(0.05)                                                             # a call whose conf_thres is below low_thres
    for kw, word in ((dict(assign='hungarian'), 'assign'), (dict(assign=1), 'assign'), (dict(low_thres=float('nan')), 'finite'),
                     (dict(low_thres=0.1, high_thres=float('inf')), 'finite'), (dict(low_thres=0.1, low_match_thres=float('nan')), 'finite'),
                     (dict(low_thres=0.5, high_thres=0.5), 'low_thres < high_thres'), (dict(low_thres=0.5, high_thres=0.4), 'low_thres < high_thres'),
                     (dict(high_thres=0.5), 'low_thres'), (dict(low_match_thres=0.5), 'low_thres')):
        with pytest.raises(ValueError, match=word):
            Tracker(**kw)
    assert t.state is None                                                        # no device was touched
    g = ops.track_assoc()
    assert (g.assign, g.bands, g.high_thres, g.low_thres, g.low_match_thres, list(g.reserved)) == (0, 0, 0.0, 0.0, 0.0, [0, 0, 0])
    for kw, word in ((dict(assign='best'), 'assign'), (dict(low_thres=0.1), 'required'), (dict(low_thres=0.1, high_thres=0.3), 'required'),
                     (dict(high_thres=0.3), 'second stage'), (dict(low_thres=0.3, high_thres=0.3, low_match_thres=0.3), 'low_thres < high_thres'),
                     (dict(low_thres=0.1, high_thres=0.3, low_match_thres=float('inf')), 'finite')):
        with pytest.raises(ValueError, match=word):
            ops.track_assoc(**kw)
    with pytest.raises(TypeError, match='TrackAssoc'):
        ops.track_frames(None, None, ops.track_params((4, 4)), assoc={'assign': 'optimal'})


def test_the_new_entry_point_is_declared_exported_and_bound():
    from mydetection_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'mydet.h')).read()
    assert re.search(r'\bint\s+mydet_track_frames_assoc_f32\s*\(', header)
    handle, lib = ctypes.CDLL(_lib.LIB_PATH), _lib.lib()
    name = 'mydet_track_frames_assoc_f32'
    assert hasattr(handle, name) and len(_lib.SIGNATURES[name]) == 18 and getattr(lib, name).argtypes == _lib.SIGNATURES[name]
    assert _lib.SIGNATURES[name][:16] == _lib.SIGNATURES['mydet_track_frames_f32'][:16]

    def define(word):
        return int(re.search(r'#define ' + word + r'\s+(-?\d+)', header).group(1))
    assert (define('MYDET_TRACK_ASSIGN_GREEDY'), define('MYDET_TRACK_ASSIGN_OPTIMAL')) == (_lib.TRACK_ASSIGN_GREEDY, _lib.TRACK_ASSIGN_OPTIMAL) == (0, 1)
    assert define('MYDET_ABI_VERSION') == _lib.ABI_VERSION == lib.mydet_abi_version() == 2          # new symbols only
    body = re.search(r'typedef struct mydet_track_assoc \{(.*?)\} mydet_track_assoc;', header, re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    fields = []
    for decl in body.split(';'):
        words = decl.split()
        if words:
            kind = {'int': ctypes.c_int, 'float': ctypes.c_float}[words[0]]
            for item in ' '.join(words[1:]).split(','):
                m = re.fullmatch(r'\s*(\w+)(?:\[(\d+)\])?\s*', item)
                fields.append((m.group(1), kind * int(m.group(2)) if m.group(2) else kind))
    assert fields == list(_lib.TrackAssoc._fields_)
    assert [f for f, _ in fields] == ['assign', 'bands', 'high_thres', 'low_thres', 'low_match_thres', 'reserved']
    assert ctypes.sizeof(_lib.TrackAssoc) == 32 and _lib.TrackAssoc.reserved.offset == 20


def test_abi_argument_checks_of_the_new_entry_point():
    """Every call below must fail before any launch: the pointers are host addresses."""
    from mydetection_amd import _lib, ops
    lib = _lib.lib()
    buf = (ctypes.c_int32 * 64)()
    p = (ctypes.cast(buf, ctypes.c_void_p).value + 15) // 16 * 16
    par = ops.track_params((480, 640))

    def call(assoc, S=2, state=p, bw=4):
        ref_ = ctypes.byref(assoc) if assoc is not None else None
        return lib.mydet_track_frames_assoc_f32(p, 3 * _lib.REC_WORDS, _lib.REC_WORDS, S, 3, bw, ctypes.byref(par), 4, state, p, p, p, p, p, p, p, ref_, None)

    def assoc(**kw):
        a = ops.track_assoc('optimal', 0.1, 0.3, 0.3)
        for k, v in kw.items():
            setattr(a, k, v)
        return a
    bad = -1
    assert call(None) == bad
    assert call(assoc(assign=2)) == bad and call(assoc(assign=-1)) == bad
    assert call(assoc(bands=2)) == bad and call(assoc(bands=-1)) == bad
    for field in ('high_thres', 'low_thres', 'low_match_thres'):
        for v in (float('nan'), float('inf'), -float('inf')):
            assert call(assoc(**{field: v})) == bad, (field, v)
    assert call(assoc(low_thres=0.3)) == bad and call(assoc(low_thres=0.5)) == bad
    # what is wrong for the entry point of old is wrong here, whatever the mode
    for a in (ops.track_assoc(), ops.track_assoc('optimal'), assoc()):
        assert call(a, S=0) == bad and call(a, state=p + 4) == bad and call(a, bw=3) == bad and call(a, state=None) == bad


def _all_cases():
    import _assoc_cases as ac
    out = {}
    for assign in ('greedy', 'optimal'):
        for variant in ('4', '5iou', '5rot'):
            out[f'ab_{variant}_{assign}'] = ac.ab_case(variant, assign)
        out[f'bands_{assign}'] = ac.bands_case(assign)
        out[f'filtered_{assign}'] = ac.bands_case(assign, bands=False)
        out[f'classes_{assign}'] = ac.classes_case(assign)
        out[f'bad_class_{assign}'] = ac.bad_class_case(dict(assign=assign))
        out[f'bad_class_{assign}_bands'] = ac.bad_class_case(dict(assign=assign, **ac.BANDS))
    out['tie_4'], out['tie_5rot'] = ac.tie_case('optimal'), ac.tie_case('optimal', '5')
    return out


@pytest.mark.parametrize('name', list(_all_cases()))
def test_hand_made_cases_on_the_restatement(name):
    """The expectations written in tests/_assoc_cases.py, in float64 and in float32, with the margins the GPU tests rely on."""
    import _assoc_cases as ac
    case = _all_cases()[name]
    for dtype in (np.float64, np.float32):
        stream, outs = aref.run_case(case, dtype, ac.IMG_HW)
        for f, (got, want) in enumerate(zip(outs, case['expect'])):
            assert all(got[k] == want[k] for k in ('id', 'missed', 'count', 'dropped')), (name, dtype.__name__, f, got, want)
        assert len(outs) == len(case['expect']) and stream.ties == case['ties']
        assert aref.margins_hold(stream), (name, stream.margins)


def test_grid_case_on_the_restatement():
    """130 tracks x 70 detections: the margins hold, every component is small enough to be enumerated, five detections per frame
    end on their dummy columns, and the greedy walk decides otherwise -- the case can tell the modes apart."""
    import _assoc_cases as ac
    case = dict(width=4, match='iou', max_tracks=ac.GRID_MT, params=ac.GRID_PARAMS, assoc=dict(assign='optimal'), frames=ac.grid_frames(1))
    stream, outs = aref.run_case(case, np.float64, ac.IMG_HW)
    assert aref.margins_hold(stream) and stream.ties == 0, stream.margins
    assert [o['count'] for o in outs] == [65, 130, 130, 130] and [o['dropped'] for o in outs] == [0, 0, 5, 5]
    assert [sum(m == 0 for m in o['missed']) for o in outs] == [65, 65, 65, 65]
    assert all(len(f[1]) <= ac.GRID_DETS for f in case['frames'])
    _, greedy = aref.run_case(dict(case, assoc=dict(assign='greedy')), np.float64, ac.IMG_HW)
    assert greedy[2]['missed'] != outs[2]['missed'] and greedy[3]['missed'] != outs[3]['missed']


def test_detector_lowers_the_calls_threshold_for_a_two_stage_tracker_only():
    """Detector._detect on a meta-device model: with low_thres the call's post-process settings carry min(conf_thres, low_thres)
    and the tracker is handed the call's own conf_thres; a conf_thres that is not above low_thres is a ValueError before any GPU
    work; without low_thres the settings are untouched."""
    from mydetection_amd.api import Tracker
    from test_track_host import _meta_detector
    det = _meta_detector()
    frames = np.zeros((2, 96, 128, 3), np.uint8)
    seen = []

    class Stop(Exception):
        pass

    def source_records(sources, call):
        seen.append(call.conf_thres)
        raise Stop
    det._source_records = source_records
    for tracker, conf, want in ((Tracker(low_thres=0.05), 0.3, 0.05), (Tracker(assign='optimal', low_thres=0.2), 0.5, 0.2),
                                (Tracker(assign='optimal'), 0.3, 0.3), (Tracker(), 0.3, 0.3), (None, 0.3, 0.3)):
        with pytest.raises(Stop):
            det.predict_frames(frames, tracker=tracker, conf_thres=conf)
        assert seen[-1] == want
    n = len(seen)
    with pytest.raises(ValueError, match='low_thres < high_thres'):
        det.predict_frames(frames, tracker=Tracker(low_thres=0.3), conf_thres=0.3)
    with pytest.raises(ValueError, match='low_thres < high_thres'):
        det.predict_frames(frames, tracker=Tracker(low_thres=0.05), conf_thres=0.001)
    assert len(seen) == n                                                         # rejected before the records were asked for
