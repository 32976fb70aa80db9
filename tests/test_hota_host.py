"""CPU: the HOTA scorer's host side.  The declarations; the argument errors for bad alphas; ops.hota_summarize on hand-made
integers; hota=False leaves the result and the summary text as they were; and the restatement tests/_hota_ref.py itself (what the
GPU tests compare the kernels with) on closed forms and against brute force."""
import ctypes
import inspect
import math
import os
import re
import types

import numpy as np
import pytest

import _hota_ref as href
import _mot_cases as cases
import _mot_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {'mydet_hota_align_f64': 7, 'mydet_hota_match': 9, 'mydet_hota_score_f64': 13}
RATIOS = ('hota', 'deta', 'assa', 'detre', 'detpr', 'assre', 'asspr', 'loca')


def test_entry_points_are_declared_exported_bound_and_documented():
    from mydetection_amd import _lib, ops
    header = open(os.path.join(ROOT, 'include', 'mydet.h')).read()
    dll = ctypes.CDLL(_lib.LIB_PATH)
    for name, nargs in NAMES.items():
        m = re.search(r'\bint\s+' + name + r'\s*\(([^;]*)\)\s*;', header)
        assert m and len(m.group(1).split(',')) == nargs, name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name]) == nargs and name not in _lib.RETURNS_I64
        assert hasattr(dll, name)
    assert (_lib.HOTA_P_ONE, _lib.HOTA_Q_ONE, _lib.HOTA_MAX_FRAMES) == (href.P_ONE, href.Q_ONE, 1 << 22) == (1 << 30, 1 << 20, 1 << 22)
    design = open(os.path.join(ROOT, 'DESIGN.md')).read()
    readme = open(os.path.join(ROOT, 'README.md')).read()
    for text in ('floor(s * 2^30)', 'rowsum[r] + colsum[c] - iou', '1048576 - q', 'floor(A * iou * 1048576.0)', 'max(1, gt_count + dt_count - M)'):
        assert text in header and text in design, text
    for text in ('HOTA', 'DetA', 'AssA', 'LocA', 'TrackEval', 'profiles/hota.md'):
        assert text in readme, text
    mk = open(os.path.join(ROOT, 'mydetection_amd', 'csrc', 'Makefile')).read()
    assert re.search(r'SRCS_EXACT\s*=.*\bhota\.hip\b', mk)
    for fn in (ops.hota_align, ops.hota_match, ops.hota_score, ops.hota_evaluate, ops.hota_summarize):
        assert callable(fn)
    from mydetection_amd.api import TrackEvaluator
    from mydetection_amd.utils.evaluation import mot
    for fn in (TrackEvaluator.__init__, mot.MOTeval.__init__, mot.evaluate_json):
        assert inspect.signature(fn).parameters['hota'].default is False
    assert np.array_equal(ops.hota_alphas(True), np.arange(1, 20) / 20.0) and href.DEFAULT_ALPHAS == ops.hota_alphas(True).tolist()


def test_bad_alphas_are_value_errors():
    from mydetection_amd import ops
    from mydetection_amd.api import TrackEvaluator
    from mydetection_amd.utils.evaluation.mot import MOTeval
    gt, rows = cases.build(cases.swap())
    for bad in ([], [0.0], [-0.5], [1.5], [0.5, float('nan')], np.linspace(0.01, 1, 33), [[0.5, 0.6]]):
        with pytest.raises(ValueError):
            ops.hota_alphas(bad)
        with pytest.raises(ValueError):
            MOTeval(gt, rows, 'coco', hota=bad)
        with pytest.raises(ValueError):
            TrackEvaluator(gt, 'coco', hota=bad)
    assert ops.hota_alphas([1.0, 0.5]).tolist() == [1.0, 0.5] and len(ops.hota_alphas(np.linspace(0.01, 1, 32))) == 32
    assert MOTeval(gt, rows, 'coco', hota=False).hota_alphas is None and len(MOTeval(gt, rows, 'coco', hota=True).hota_alphas) == 19
    assert TrackEvaluator(gt, 'coco', hota=(0.5,)).hota.tolist() == [0.5] and TrackEvaluator(gt, 'coco').hota is False


def test_summary_arithmetic_from_hand_made_integers():
    from mydetection_amd import ops
    m = ops.hota_metrics(tp=6, fn=2, fp=4, loc_sum=4.5, ass_sum=(3.0, 4.5, 1.5))
    assert m['deta'] == 0.5 and m['detre'] == 0.75 and m['detpr'] == np.float64(6) / np.float64(10)
    assert (m['assa'], m['assre'], m['asspr'], m['loca']) == (0.5, 0.75, 0.25, 0.75) and m['hota'] == 0.5
    zero = ops.hota_metrics(0, 0, 0, 0.0, (0.0, 0.0, 0.0))
    assert zero['loca'] == 1.0 and all(zero[k] == 0.0 for k in RATIOS if k != 'loca')
    assert ops.hota_metrics(0, 3, 0, 0.0, (0.0, 0.0, 0.0))['detre'] == 0.0
    # S = 2, K = 1, T = 2
    pack = {'S': 2, 'K': 1, 'seq_names': ['a', 'b']}
    raw = {'counts': np.array([[[4, 0, 0], [2, 2, 2]], [[2, 2, 4], [0, 4, 6]]]), 'loc_sum': np.array([[3.0, 2.0], [1.5, 0.0]]),
           'ass_sum': np.array([[[4.0, 4.0, 4.0], [1.0, 2.0, 1.0]], [[1.0, 1.0, 2.0], [0.0, 0.0, 0.0]]])}
    result, text = ops.hota_summarize(raw, pack, np.array([0.25, 0.75]))
    a, b, o = result['sequences']['a'], result['sequences']['b'], result['overall']
    assert result['alphas'] == [0.25, 0.75] and list(result['sequences']) == ['a', 'b']
    assert a['per_alpha']['tp'] == [4, 2] and a['per_alpha']['deta'] == [1.0, np.float64(2) / np.float64(6)] and a['per_alpha']['assa'] == [1.0, 0.5]
    assert a['per_alpha']['loca'] == [0.75, 1.0] and a['hota0'] == 1.0 and a['loca0'] == 0.75 and a['hota_loca0'] == 0.75
    assert a['deta'] == float(np.mean(np.array(a['per_alpha']['deta']))) and a['hota'] == float(np.mean(np.array(a['per_alpha']['hota'])))
    assert b['per_alpha']['deta'] == [0.25, 0.0] and b['per_alpha']['assa'] == [0.5, 0.0] and b['per_alpha']['loca'] == [0.75, 1.0]
    assert b['per_alpha']['hota'] == [float(np.sqrt(np.float64(0.125))), 0.0]
    assert o['per_alpha']['tp'] == [6, 2] and o['per_alpha']['fn'] == [2, 6] and o['per_alpha']['fp'] == [4, 8]
    assert o['per_alpha']['deta'] == [0.5, 0.125] and o['per_alpha']['assa'] == [np.float64(5) / np.float64(6), 0.5]
    assert o['per_alpha']['loca'] == [0.75, 1.0]
    lines = text.splitlines()
    assert len(lines) == 4 and lines[0].split()[:4] == ['sequence', 'hota', 'deta', 'assa'] and lines[3].split()[0] == 'OVERALL'
    assert lines[3].split()[2] == '0.3125' and lines[1].split()[0] == 'a'
    # the restatement's summary agrees on the same arrays
    r = href.summarize({'S': 2, 'K': 1, 'seq_names': ['a', 'b'], 'alphas': [0.25, 0.75], **raw})
    for got, want in ((a, r['sequences']['a']), (b, r['sequences']['b']), (o, r['overall'])):
        assert got['per_alpha']['tp'] == want['per_alpha']['tp']
        for k in RATIOS:
            assert np.allclose(got['per_alpha'][k], want['per_alpha'][k], rtol=1e-15, atol=0) and abs(got[k] - want[k]) <= 1e-15


def _host_eval(scene, hota, n_cats=1):
    """MOTeval.summarize() on the restatements' arrays as CPU tensors: the host half of the class without a device."""
    torch = pytest.importorskip('torch')
    from mydetection_amd import ops
    from mydetection_amd.utils.evaluation.mot import MOTeval
    gt, rows = cases.build(scene, n_cats=n_cats)
    e = MOTeval(gt, rows, 'coco', (0.5,), hota=hota)
    e.packed = types.SimpleNamespace(pack=ops.mot_pack(rows, gt, 'coco'))
    r = ref.evaluate(rows, gt, 'coco', [0.5])
    e.tensors = {k: torch.from_numpy(np.ascontiguousarray(r[k])) for k in ('counts', 'siou', 'present', 'matched', 'idtp', 'ious', 'overlap')}
    e.tensors['gt_match'] = None
    if e.hota_alphas is not None:
        h = href.evaluate(rows, gt, 'coco', e.hota_alphas)
        e.hota_tensors = {k: torch.from_numpy(np.ascontiguousarray(h[k])) for k in ('ious', 'pot', 'gt_count', 'dt_count', 'score_q', 'hota_match',
                                                                                  'counts', 'matches', 'loc_sum', 'ass_sum')}
    e.summarize()
    return e


def test_hota_off_leaves_the_result_and_the_summary_as_they_were():
    from mydetection_amd import ops
    scene = cases.several()
    off = _host_eval(scene, False, n_cats=2)
    want, text = ops.mot_summarize(off.raw, off.packed.pack, off.iou_thrs)
    assert set(off.result) == {'iou_thrs', 'overall', 'sequences'} and off.result == want and off.summary == text
    assert 'hota' not in off.summary and 'hota' not in off.raw
    on = _host_eval(scene, True, n_cats=2)
    assert set(on.result) == {'iou_thrs', 'overall', 'sequences', 'hota'} and {k: v for k, v in on.result.items() if k != 'hota'} == want
    assert on.summary.startswith(text) and on.summary[len(text):].splitlines()[0].split()[:2] == ['sequence', 'hota']
    assert on.summary.count('\n') == text.count('\n') + 1 + 4
    h = on.result['hota']
    assert set(h) == {'alphas', 'overall', 'sequences'} and len(h['alphas']) == 19 and list(h['sequences']) == [0, 1, 2]
    assert set(h['overall']) == {'per_alpha', 'hota0', 'loca0', 'hota_loca0'} | set(RATIOS) and len(h['overall']['per_alpha']['hota']) == 19
    assert 0 < h['overall']['hota'] < 1 and 0 < h['overall']['assa'] < 1 and set(on.raw['hota']) >= {'pot', 'score_q', 'hota_match'}


def _overall(scene, alphas=None, **kw):
    gt, rows = cases.build(scene)
    r = href.evaluate(rows, gt, 'coco', alphas, **kw)
    return r, href.summarize(r)['overall']


def test_reference_perfect_tracker_scores_one_at_every_alpha():
    scene = [[(gts, [(100 + g[0], g[1]) for g in gts]) for gts, _ in seq] for seq in cases.several(K=1)]
    r, o = _overall(scene)
    for k in RATIOS:
        assert o['per_alpha'][k] == [1.0] * 19 and o[k] == 1.0, k
    assert (r['counts'][:, :, 1:] == 0).all() and (r['hota_match'] == np.arange(r['G'])).all() and o['hota_loca0'] == 1.0
    assert r['score_q'].max() == href.Q_ONE and (r['pot'] <= int(r['gt_count'].max()) * href.P_ONE).all()


def test_reference_without_hypotheses_scores_zero():
    scene = [[(gts, []) for gts, _ in seq] for seq in cases.several(K=1)]
    r, o = _overall(scene)
    for k in RATIOS:
        assert o[k] == (1.0 if k == 'loca' else 0.0), k
    assert (r['counts'][:, :, 0] == 0).all() and (r['counts'][:, :, 2] == 0).all() and r['counts'][:, 0, 1].sum() == r['G'] > 0
    assert (r['hota_match'] == -1).all() and r['score_q'].size == 0 and r['pot'].size == 0
    # and without ground truth
    r, o = _overall([[([], hyps) for _, hyps in seq] for seq in cases.several(K=1)])
    assert o['hota'] == 0.0 and o['deta'] == 0.0 and r['counts'][:, 0, 2].sum() == r['D'] > 0


@pytest.mark.parametrize('k', [1, 3, 8])
def test_reference_one_object_under_two_identities(k):
    a = cases.box(0)
    scene = [[([(1, a)], [(1, a)])] * k + [([(1, a)], [(2, a)])] * k]
    r, o = _overall(scene)
    assert o['per_alpha']['deta'] == [1.0] * 19 and o['per_alpha']['assa'] == [0.5] * 19 and o['per_alpha']['loca'] == [1.0] * 19
    assert o['per_alpha']['hota'] == [math.sqrt(0.5)] * 19 and o['assre'] == 0.5 and o['asspr'] == 1.0
    assert r['matches'][0].tolist() == [k, k] and r['gt_count'].tolist() == [2 * k] and r['dt_count'].tolist() == [k, k]
    assert r['pot'].tolist() == [k * href.P_ONE] * 2 and r['score_q'].tolist() == [href.Q_ONE // 2] * (2 * k)


def test_reference_assignment_total_equals_brute_force_on_pair_scores():
    rng = np.random.default_rng(7)
    shapes = set()
    for n in range(200):
        n_rows, n_cols = int(rng.integers(1, 7)), int(rng.integers(1, 8))
        iou = rng.random((n_cols, n_rows)) * (rng.random((n_cols, n_rows)) < 0.7)
        if n % 4 == 0:
            iou = np.round(iou * 4) / 4                               # equal scores: ties
        frames = 1 + int(rng.integers(0, 5))
        P = rng.integers(0, frames * href.P_ONE + 1, (n_rows, n_cols)) * (rng.random((n_rows, n_cols)) < 0.8)
        q = href.pair_scores(iou, P.tolist(), [frames] * n_rows, [frames] * n_cols)
        assert q.min() >= 0 and q.max() <= href.Q_ONE
        cost = href.Q_ONE - q.T
        col_of_row, total = ref.assign(cost)
        used = [c for c in col_of_row if c >= 0]
        assert len(used) == min(cost.shape) and len(set(used)) == len(used) and total == ref.brute_force(cost), cost
        shapes.add(cost.shape)
    assert (6, 7) in shapes and (1, 1) in shapes and any(a > b for a, b in shapes)
