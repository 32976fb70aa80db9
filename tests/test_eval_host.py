"""CPU-only: the host side of the evaluator -- the numpy restatement (tests/_eval_ref.py) against hand-computed anchors and against
the rule each case of tests/_eval_cases.py isolates, the packer and the summary of the package against the restatement, and the
C ABI (declared, exported, bound, constants, the ABI version unchanged, every argument check before any launch)."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

import _eval_cases as cases
import _eval_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {'mydet_eval_ious_f64': 3, 'mydet_eval_match_f64': 10, 'mydet_eval_accumulate_f64': 17}
_CACHE = {}


def _ref(name):
    if name not in _CACHE:
        gt, dts, params = cases.CASES[name]()
        _CACHE[name] = ref.evaluate(dts, gt, 'coco', params)
    return _CACHE[name]


SUMMARY_FP_THEN_TP = (
    ' Average Precision  (AP) @[ IoU=0.50:0.95 | area=   all | maxDets=100 ] = 0.500\n'
    ' Average Precision  (AP) @[ IoU=0.50      | area=   all | maxDets=100 ] = 0.500\n'
    ' Average Precision  (AP) @[ IoU=0.75      | area=   all | maxDets=100 ] = 0.500\n'
    ' Average Precision  (AP) @[ IoU=0.50:0.95 | area= small | maxDets=100 ] = 0.500\n'
    ' Average Precision  (AP) @[ IoU=0.50:0.95 | area=medium | maxDets=100 ] = -1.000\n'
    ' Average Precision  (AP) @[ IoU=0.50:0.95 | area= large | maxDets=100 ] = -1.000\n'
    ' Average Recall     (AR) @[ IoU=0.50:0.95 | area=   all | maxDets=  1 ] = 0.000\n'
    ' Average Recall     (AR) @[ IoU=0.50:0.95 | area=   all | maxDets= 10 ] = 1.000\n'
    ' Average Recall     (AR) @[ IoU=0.50:0.95 | area=   all | maxDets=100 ] = 1.000\n'
    ' Average Recall     (AR) @[ IoU=0.50:0.95 | area= small | maxDets=100 ] = 1.000\n'
    ' Average Recall     (AR) @[ IoU=0.50:0.95 | area=medium | maxDets=100 ] = -1.000\n'
    ' Average Recall     (AR) @[ IoU=0.50:0.95 | area= large | maxDets=100 ] = -1.000\n')


def _fp_then_tp():
    gt = cases.gt_set(1, 1, [cases.ann(0, 0, [0, 0, 10, 10])])
    return gt, [cases.det(0, 0, [100, 100, 10, 10], .9), cases.det(0, 0, [0, 0, 10, 10], .8)]


def test_anchor_false_positive_then_true_positive():
    gt, dts = _fp_then_tp()
    r = ref.evaluate(dts, gt, 'coco')
    assert abs(r['stats'][1] - 0.5) <= 1e-12 and abs(r['stats'][0] - 0.5) <= 1e-12
    assert r['stats'][8] == 1.0 and r['stats'][7] == 1.0 and r['stats'][6] == 0.0
    assert r['summary'] == SUMMARY_FP_THEN_TP
    assert (r['precision'][:, :, 0, 0, 2] == 1 / (2 + 2.0 ** -52)).all() and (r['scores'][:, 1:, 0, 0, 2] == .8).all()
    assert (r['scores'][:, 0, 0, 0, 2] == .9).all()                  # recall 0 is reached by the first detection


def test_anchor_perfect_detections():
    boxes = ([0, 0, 20, 20], [100, 0, 50, 50], [200, 200, 200, 200], [0, 300, 10, 30])
    gt = cases.gt_set(2, 2, [cases.ann(n % 2, n // 2, b) for n, b in enumerate(boxes)])
    dts = [cases.det(n % 2, n // 2, b, .9 - .1 * n) for n, b in enumerate(boxes)]
    r = ref.evaluate(dts, gt, 'coco')
    assert (r['stats'] > -1).all() and np.abs(r['stats'] - 1).max() <= 1e-12
    assert (r['ious'] == 1.0).all() and len(r['ious']) == 4


def test_each_case_shows_its_rule():
    r = _ref('threshold_hit_exactly')
    assert list(r['ious']) == [0.5, 0.75] and r['matched'][0, 0] == 0b1 and r['matched'][0, 1] == 0b111111
    r = _ref('threshold_above_the_cap')
    assert r['ious'][0] == 1.0 and 0.98 < r['ious'][3] < 1 and list(r['matched'][0]) == [0b11, 0b01]
    r = _ref('equal_iou_later_wins')
    assert list(r['gt_row'][0, 0]) == [1, 0, -1] and list(r['matched'][0]) == [1023, 1023, 0]
    r = _ref('crowd_matched_by_several')
    assert list(r['ious'][0:6:2]) == [1.0, 1.0, 1.0] and list(r['gt_row'][0, 0]) == [0, 0, 0, 1, -1]
    assert list(r['ignored'][0]) == [1023, 1023, 1023, 0, 0] and 0 < r['ious'][8] < 0.5         # i/da of a box half outside the crowd
    r = _ref('non_ignored_match_stops_the_walk')
    assert r['gt_row'][0, 0, 0] == 0 and r['gt_row'][1, 0, 0] == 1 and r['ignored'][1, 0] == 0b1111110000 and r['matched'][1, 0] == 0b1111111
    assert list(r['gt_row'][1, :5, 0]) == [1, 1, 1, 1, 0]                              # the ignored one only where the other fails
    r = _ref('ignored_match_stays')
    assert list(r['gt_row'][1, :4, 0]) == [1, 1, 0, 0] and r['ignored'][1, 0] & 0b1111 == 0b1100 and r['matched'][1, 0] == 0b1111111
    r = _ref('ground_truth_outside_each_range')
    assert [list(r['ignored'][a] != 0) for a in range(4)] == [[False] * 5, [False, True, True, False, True], [True, False, True, False, False],
                                                              [True, True, False, True, False]]
    assert (r['matched'] == 1023).all()
    r = _ref('unmatched_detection_outside_the_range')
    assert list(r['ignored'][0]) == [0] * 4 and list(r['matched'][0]) == [0, 0, 0, 1023]
    assert list(r['ignored'][1]) == [0, 1023, 1023, 0] and list(r['ignored'][2]) == [1023, 0, 1023, 1023] and list(r['ignored'][3]) == [1023, 1023, 0, 1023]
    r = _ref('boxes_that_only_touch')
    assert (r['ious'] == 0).all() and (r['matched'] == 0).all()
    r = _ref('zero_area_boxes')
    assert list(r['ious']) == [0, 0, 0, 0, 1, 0] and not np.isnan(r['ious']).any() and list(r['matched'][0]) == [0, 0, 1023]
    r = _ref('more_detections_than_max_dets')
    assert r['D'] == 100 and r['recall'][0, 0, 0, 2] == 0.5 and .4 not in r['dt_score'] and r['dt_score'].min() == .5 + .004 * 4
    r = _ref('one_sided_groups')
    assert list(r['listed']) == [0, 1, 2] and len(r['ious']) == 1 and r['recall'][0, 0, 0, 2] == 0.5
    r = _ref('category_without_ground_truth')
    assert (r['precision'][:, :, 1:] == -1).all() and (r['recall'][:, 1:] == -1).all() and (r['scores'][:, :, 2] == -1).all()
    assert (r['precision'][:, :, 0, 0] > 0.99).all() and r['D'] == 2
    r = _ref('ground_truth_without_detections')
    assert (r['recall'][:, 1, 0] == 0).all() and (r['precision'][:, :, 1, 0] == 0).all() and (r['precision'][:, :, 1, 2] == -1).all()
    r = _ref('recall_stops_short')
    assert r['recall'][0, 0, 0, 2] == 0.5 and (r['precision'][0, 51:, 0, 0, 2] == 0).all() and (r['precision'][0, :51, 0, 0, 2] > 0).all()
    assert (r['scores'][0, 51:, 0, 0, 2] == 0).all()
    r = _ref('score_ties_across_images')
    assert list(r['order']) == [0, 2, 3, 1] and abs(r['stats'][1] - 0.75) < 1e-9       # input order would give 1 at low recall
    r = _ref('ground_truths_1024')
    assert r['G'] == 1024 and list(r['gt_row'][0, 0]) == [1023, 1022, 0, -1] and list(r['gt_row'][0, 9]) == [1023, -1, 0, -1]
    with pytest.raises(AssertionError, match='more ground truths'):
        ref.evaluate(*cases.ground_truths_1025()[1::-1], 'coco')


def _sets():
    for name, make in cases.CASES.items():
        yield (name, 'coco') + make()
    yield ('mixed', 'coco') + cases.mixed_set()
    yield ('rotated', 'cepdof') + cases.rotated_set()


@pytest.mark.parametrize('case', list(_sets()), ids=lambda c: c[0])
def test_packer_gives_the_documented_layout(case):
    from mydetection_amd import ops
    name, kind, gt, dts, params = case
    r = ref.evaluate(dts, gt, kind, params) if name not in cases.CASES else _ref(name)
    p = ops.eval_pack(dts, gt, kind, 100)
    assert (p['I'], p['K'], p['D'], p['G'], p['n_pairs']) == (r['I'], r['K'], r['D'], r['G'], len(r['ious']))
    for key in ('dt_start', 'gt_start', 'dt_rows', 'gt_rows', 'dt_score', 'dt_area', 'gt_area', 'gt_flags', 'dt_rank', 'order', 'cat_start'):
        assert np.array_equal(p[key], r[key]), key
    assert np.array_equal(p['groups'], r['listed'])
    for key, dtype in (('dt_start', np.int32), ('gt_start', np.int32), ('groups', np.int32), ('pair_start', np.int64), ('dt_score', np.float64),
                       ('dt_area', np.float64), ('gt_area', np.float64), ('gt_flags', np.uint8), ('order', np.int32), ('dt_rank', np.int32),
                       ('dt_box', np.float32 if kind == 'cepdof' else np.float64)):
        assert p[key].dtype == dtype and p[key].flags['C_CONTIGUOUS'], key
    width = 5 if kind == 'cepdof' else 4
    assert p['dt_box'].shape == (p['D'], width) and p['gt_box'].shape == (p['G'], width)
    assert np.array_equal(p['dt_box'], np.array([dts[n]['bbox'][:width] for n in p['dt_rows']], p['dt_box'].dtype).reshape(-1, width))
    assert np.array_equal(p['gt_box'], np.array([gt['annotations'][n]['bbox'][:width] for n in p['gt_rows']], p['gt_box'].dtype).reshape(-1, width))
    nd, ng = np.diff(p['dt_start'].astype(np.int64)), np.diff(p['gt_start'].astype(np.int64))
    assert np.array_equal(np.diff(p['pair_start']), (nd * ng)[p['groups']]) and p['pair_start'][0] == 0
    assert p['max_dt'] == nd.max(initial=0) and p['max_gt'] == ng.max(initial=0)
    # the same through the columns, and the summary of the package on the restatement's arrays
    q = ops.eval_pack(ops.eval_columns(dts, kind), gt, kind, 100)
    assert all(np.array_equal(p[k], q[k]) for k in p if isinstance(p[k], np.ndarray))
    prm = ops.EvalParams()
    for k, v in (params or {}).items():
        setattr(prm, k, v)
    stats, summary = ops.eval_summarize(r['precision'], r['recall'], prm)
    assert np.array_equal(stats, r['stats']) and summary == r['summary']


def test_mixed_and_rotated_sets_have_what_they_promise():
    gt, dts, _ = cases.mixed_set()
    r = ref.evaluate(dts, gt, 'coco')
    assert r['D'] < len(dts) and (r['gt_flags'] & 2).any() and len(set(r['dt_score'])) < r['D'] / 2 and len(r['listed']) < r['I'] * r['K']
    assert (r['stats'][:3] > 0).all() and (r['stats'][:3] < 1).all() and (r['ignored'] != 0).any() and (r['matched'] != 0).any()
    gt, dts, _ = cases.rotated_set()
    r = ref.evaluate(dts, gt, 'cepdof')
    assert r['K'] == 1 and (r['gt_flags'] & 1).any() and 0 < r['stats'][0] < 1 and ((r['ious'] > 0.5) & (r['ious'] < 0.95)).sum() > 10


def test_params_defaults_and_summary_text_of_the_package():
    from mydetection_amd import ops
    p, d = ops.EvalParams(), ref.default_params()
    assert np.array_equal(p.iouThrs, d['iouThrs']) and np.array_equal(p.recThrs, d['recThrs']) and p.maxDets == d['maxDets']
    assert np.array_equal(np.asarray(p.areaRng, np.float64), np.asarray(d['areaRng'], np.float64)) and p.areaRngLbl == list(ref.LABELS)
    gt, dts = _fp_then_tp()
    r = ref.evaluate(dts, gt, 'coco')
    assert ops.eval_summarize(r['precision'], r['recall'], p)[1] == SUMMARY_FP_THEN_TP
    with pytest.raises(ValueError):
        ops.eval_pack(dts, gt, 'segm')
    with pytest.raises(ValueError):
        ops.eval_pack(dts, {'images': [], 'categories': [], 'annotations': []}, 'coco')


def _header():
    return open(os.path.join(ROOT, 'include', 'mydet.h')).read()


def test_entry_points_are_declared_exported_and_bound():
    from mydetection_amd import _lib
    header = _header()
    dll = ctypes.CDLL(_lib.LIB_PATH)
    for name, nargs in NAMES.items():
        assert re.search(r'\bint\s+' + name + r'\s*\(', header)
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name]) == nargs
        assert hasattr(dll, name)
        assert getattr(_lib.lib(), name).argtypes == _lib.SIGNATURES[name]
    for name, value in (('MYDET_EVAL_MAX_GT', 1024), ('MYDET_EVAL_MAX_DT', 1024), ('MYDET_EVAL_MAX_THRS', 32), ('MYDET_EVAL_MAX_AREAS', 8),
                        ('MYDET_EVAL_MAX_DETS', 8), ('MYDET_EVAL_MAX_RECS', 128), ('MYDET_EVAL_GT_IGNORE', 1), ('MYDET_EVAL_GT_CROWD', 2)):
        assert re.search(r'#define\s+' + name + r'\s+' + str(value) + r'\b', header)
        assert getattr(_lib, name[len('MYDET_'):]) == value
    assert (ref.IGNORE, ref.CROWD) == (_lib.EVAL_GT_IGNORE, _lib.EVAL_GT_CROWD)
    assert 'typedef struct mydet_eval_set' in header
    assert re.search(r'#define\s+MYDET_ABI_VERSION\s+2\b', header) and _lib.ABI_VERSION == 2 and _lib.lib().mydet_abi_version() == 2
    s = _lib.EvalSet
    assert ctypes.sizeof(s) == 128 and s.D.offset == 24 and s.n_pairs.offset == 40 and s.groups.offset == 48 and s.gt_flags.offset == 120
    design = open(os.path.join(ROOT, 'DESIGN.md')).read()
    for text in ('min(t, 1 - 1e-10)', 'tp/(fp + tp + 2^-52)', 'fmin(dx+dw, gx+gw) - fmax(dx, gx)', 'g = k*I + i'):
        assert text in header and text in design, text
    mk = open(os.path.join(ROOT, 'mydetection_amd', 'csrc', 'Makefile')).read()
    assert re.search(r'SRCS_EXACT\s*=.*\bevalmatch\.hip\b', mk)
    from mydetection_amd.api import Evaluator                                      # noqa: F401
    from mydetection_amd.utils.evaluation import coco, cepdof
    assert callable(coco.coco_evaluate_bbox) and callable(cepdof.evaluate_json) and coco.myCOCOeval.kind == 'coco' and cepdof.CEPDOFeval.kind == 'cepdof'


def test_abi_argument_checks_come_before_any_launch():
    """Every call below must fail its checks: all pointers are host pointers and nothing may be launched on them."""
    from mydetection_amd import _lib, ops
    lib = _lib.lib()
    null = ctypes.c_void_p(0)
    gt, dts, _ = cases.mixed_set()
    pack = ops.eval_pack(dts, gt, 'coco', 100)
    p = ops.EvalParams()
    thr, rng, rec = np.ascontiguousarray(p.iouThrs), np.ascontiguousarray(np.asarray(p.areaRng, np.float64)), np.ascontiguousarray(p.recThrs)
    md = np.asarray(p.maxDets, np.int32)
    buf = np.zeros(max(pack['n_pairs'], 4 * pack['D']) + 8, np.float64)
    here = ctypes.c_void_p(buf.ctypes.data)

    def good():
        return ops.eval_set_struct(pack, {k: pack[k].ctypes.data for k in ops.EVAL_SET_ARRAYS})

    def ious(s, out=here):
        return lib.mydet_eval_ious_f64(ctypes.byref(s) if s is not None else null, out, null)

    def match(s, io=here, t=thr, T=10, r=rng, A=4, m=here, i=here):
        ptr = lambda a: a if isinstance(a, ctypes.c_void_p) else ctypes.c_void_p(a.ctypes.data)          # noqa: E731
        return lib.mydet_eval_match_f64(ctypes.byref(s) if s is not None else null, io, ptr(t), T, ptr(r), A, m, i, null, null)

    def acc(s, order=here, cs=here, rank=here, m=here, i=here, T=10, r=rng, A=4, d=md, M=3, rc=rec, R=101, pr=here, re_=here, sc=here):
        ptr = lambda a: a if isinstance(a, ctypes.c_void_p) else ctypes.c_void_p(a.ctypes.data)          # noqa: E731
        return lib.mydet_eval_accumulate_f64(ctypes.byref(s) if s is not None else null, order, cs, rank, m, i, T, ptr(r), A, ptr(d), M, ptr(rc), R,
                                             pr, re_, sc, null)

    calls = (ious, match, acc)
    assert all(f(None) == -1 for f in calls)
    for field, value in (('rotated', 2), ('rotated', -1), ('I', 0), ('K', 0), ('I', 1 << 30), ('D', -1), ('G', -1), ('n_groups', -1), ('n_pairs', -1),
                         ('max_dt', -1), ('max_gt', -1), ('D', 1 << 31), ('G', 1 << 31), ('n_groups', pack['I'] * pack['K'] + 1), ('n_groups', 0),
                         ('max_dt', pack['D'] + 1), ('max_gt', pack['G'] + 1), ('n_pairs', pack['D'] * pack['G'] + 1), ('dt_start', None),
                         ('gt_start', None), ('groups', None), ('pair_start', None), ('dt_box', None), ('dt_score', None), ('dt_area', None),
                         ('gt_box', None), ('gt_area', None), ('gt_flags', None)):
        s = good()
        setattr(s, field, value)
        assert [f(s) for f in calls] == [-1, -1, -1], (field, value)
    for field in ('max_gt', 'max_dt'):
        s = good()
        s.D, s.G = 5000, 5000
        setattr(s, field, 1025)
        assert [f(s) for f in calls] == [-2, -2, -2], field
    g1025, d1025, _ = cases.ground_truths_1025()
    big = ops.eval_pack(d1025, g1025, 'coco', 100)
    assert big['max_gt'] == 1025
    s = ops.eval_set_struct(big, {k: big[k].ctypes.data for k in ops.EVAL_SET_ARRAYS})
    assert [f(s) for f in calls] == [-2, -2, -2]

    assert ious(good(), out=null) == -1
    nan, bad_rng, bad_rng2 = np.array([.5, np.nan]), rng.copy(), rng.copy()
    bad_rng[1] = [5, 4]
    bad_rng2[2, 0] = np.nan
    assert match(good(), io=null) == -1 and match(good(), m=null) == -1 and match(good(), i=null) == -1 and match(good(), t=null) == -1
    assert match(good(), r=null) == -1 and match(good(), T=0) == -1 and match(good(), A=0) == -1 and match(good(), t=nan, T=2) == -1
    assert match(good(), r=bad_rng) == -1 and match(good(), r=bad_rng2) == -1
    assert match(good(), t=np.linspace(0, 1, 33), T=33) == -2 and match(good(), r=np.tile(rng, (3, 1)), A=9) == -2

    for kw in (dict(order=null), dict(cs=null), dict(rank=null), dict(m=null), dict(i=null), dict(r=null), dict(d=null), dict(rc=null), dict(pr=null),
               dict(re_=null), dict(sc=null), dict(T=0), dict(A=0), dict(M=0), dict(R=0), dict(r=bad_rng), dict(r=bad_rng2),
               dict(d=np.array([1, 100, 10], np.int32)), dict(d=np.array([0, 10, 100], np.int32)), dict(rc=rec[::-1].copy()),
               dict(rc=np.array([0, np.nan, 1]), R=3)):
        assert acc(good(), **kw) == -1, kw
    for kw in (dict(T=33), dict(r=np.tile(rng, (3, 1)), A=9), dict(d=np.arange(1, 10, dtype=np.int32), M=9), dict(rc=np.linspace(0, 1, 129), R=129),
               dict(d=np.array([1, 10, 1025], np.int32))):
        assert acc(good(), **kw) == -2, kw


def test_python_argument_rules_touch_no_device(tmp_path):
    import torch
    from mydetection_amd import ops
    from mydetection_amd.api import Evaluator
    from mydetection_amd.utils.evaluation import coco
    from mydetection_amd.utils.structures import ImageObjects
    gt, dts = _fp_then_tp()
    path = tmp_path / 'gt.json'
    path.write_text(json.dumps(gt))
    e = coco.myCOCOeval(str(path), dts, 'bbox', False)
    assert e.params.imgIds == [10] and e.params.catIds == [1] and e.gt_json == gt
    with pytest.raises(NotImplementedError):
        coco.myCOCOeval(gt, dts, 'segm')
    with pytest.raises(Exception, match='evaluate'):
        e.accumulate()
    with pytest.raises(Exception, match='accumulate'):
        e.summarize()
    with pytest.raises(ValueError):
        Evaluator(gt, kind='keypoints')
    ev = Evaluator(str(path), catIdx2id=[1])
    ev.add_json(dts)
    boxes = torch.tensor([[5.5, 7.25, 3.0, 4.5]])
    ev.add(ImageObjects(boxes, torch.zeros(1, dtype=torch.int64), None, torch.tensor([0.7]), 'cxcywh'), 10)
    c = ev.columns()
    assert len(ev) == 3 and c['category_id'] == [1, 1, 1] and list(c['bbox'][2]) == [4.0, 5.0, 3.0, 4.5] and c['area'][2] == 13.5
    assert c['score'][2] == float(np.float32(0.7))
    with pytest.raises(ValueError):
        ev.add(ImageObjects(torch.zeros((1, 5)), torch.zeros(1, dtype=torch.int64), None, torch.ones(1), 'cxcywhd'), 10)
    with pytest.raises(ValueError):
        ev.add([], [10])
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match='no GPU'):
            ev.result()
        with pytest.raises(RuntimeError, match='no GPU'):
            ops.EvalSet(ops.eval_pack(dts, gt, 'coco'))


def test_the_three_kernels_use_no_scratch_memory():
    """The private segment of every evaluator kernel in the built library's code-object metadata is 0 (read the way
    tests/test_wino4_no_scratch.py reads it)."""
    import importlib.util
    from mydetection_amd import _lib
    if not os.path.exists('/opt/rocm/lib/llvm/bin/llvm-readelf'):
        pytest.skip('no llvm-readelf on this machine')
    spec = importlib.util.spec_from_file_location('check_store_hazard', os.path.join(ROOT, 'tools', 'check_store_hazard.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    sizes = {}
    for _, text in mod.code_objects(_lib.LIB_PATH, notes=True):
        name = None
        for line in text.splitlines():
            m = re.match(r'\s*\.name:\s+(\S+)', line)
            if m:
                name = m.group(1)
            m = re.match(r'\s*\.private_segment_fixed_size:\s+(\d+)', line)
            if m and name and re.search(r'eval_(ious|match|accumulate)_kernel', name):
                sizes[re.search(r'eval_(ious|match|accumulate)_kernel', name).group(0)] = int(m.group(1))
    assert sizes == {'eval_ious_kernel': 0, 'eval_match_kernel': 0, 'eval_accumulate_kernel': 0}
