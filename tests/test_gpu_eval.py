"""GPU: the evaluator's three launches against the numpy restatement (tests/_eval_ref.py).  Axis-aligned sets are compared with
== throughout -- the IoU buffer, both masks, the matched rows, precision, recall, scores, the 12 stats and the text -- because that
path is float64 and integer on both sides.  The rotated set first shows, on the CPU, that no reference IoU lies within MARGIN of
a threshold, then asks for the same equality of everything behind the IoU and for the IoU itself within IOU_ATOL."""
import copy
import os
import re

import numpy as np
import pytest
import torch

import _eval_cases as cases
import _eval_ref as ref

pytestmark = pytest.mark.gpu

IOU_ATOL = 1e-5         # tests/test_gpu_rotnms.py: the float32 device function against the float64 checker
MARGIN = 1e-4
_REFS = {}


def _reference(name, kind, gt, dts, params):
    if name not in _REFS:
        _REFS[name] = ref.evaluate(dts, gt, kind, params)
    return _REFS[name]


def _run(kind, gt, dts, params):
    from mydetection_amd.utils.evaluation import cepdof, coco
    cls = cepdof.CEPDOFeval if kind == 'cepdof' else coco.myCOCOeval
    e = cls(copy.deepcopy(gt), copy.deepcopy(dts), 'bbox', False, keep_rows=True)
    for k, v in (params or {}).items():
        setattr(e.params, k, v)
    e.evaluate()                                  # every launch's return code is checked by ops (MydetError otherwise)
    e.accumulate()
    e.summarize()
    torch.cuda.synchronize()
    return e


def _same_after_the_ious(e, r):
    m = e.matches
    assert np.array_equal(m['matched'].cpu().numpy().view(np.uint32), r['matched'])
    assert np.array_equal(m['ignored'].cpu().numpy().view(np.uint32), r['ignored'])
    assert np.array_equal(m['gt_row'].cpu().numpy(), r['gt_row'])
    for key in ('precision', 'recall', 'scores'):
        assert e.eval[key].shape == r[key].shape and np.array_equal(e.eval[key], r[key]), key
    assert np.array_equal(e.stats, r['stats']) and e.summary == r['summary']
    assert e.eval['counts'] == list(r['precision'].shape)


def _axis_sets():
    for name, make in cases.CASES.items():
        yield (name,) + make()
    yield ('mixed',) + cases.mixed_set()


@pytest.mark.parametrize('case', list(_axis_sets()), ids=lambda c: c[0])
def test_axis_aligned_sets_equal_the_restatement(case):
    name, gt, dts, params = case
    r = _reference(name, 'coco', gt, dts, params)
    e = _run('coco', gt, dts, params)
    got = e.matches['ious'].cpu().numpy()
    assert got.dtype == np.float64 and np.array_equal(got, r['ious'])
    _same_after_the_ious(e, r)
    # pycocotools' ious: one [detections, ground truths] block per group
    p = e.packed.pack
    img, cat = p['img_ids'][0], p['cat_ids'][0]
    nd, ng = p['dt_start'][1] - p['dt_start'][0], p['gt_start'][1] - p['gt_start'][0]
    block = e.ious[img, cat]
    assert (len(block) == 0) if nd == 0 and ng == 0 else (block.shape == (nd, ng) and np.array_equal(block.ravel(), r['ious'][:nd * ng]))


def test_a_group_of_1025_ground_truths_is_refused():
    from mydetection_amd import _lib, ops
    gt, dts, _ = cases.ground_truths_1025()
    es = ops.EvalSet(ops.eval_pack(dts, gt, 'coco'))
    with pytest.raises(_lib.MydetError, match='unsupported'):
        ops.eval_ious(es)
    with pytest.raises(_lib.MydetError, match='unsupported'):
        ops.eval_match(es, torch.zeros(es.pack['n_pairs'], dtype=torch.float64, device='cuda'), [.5], [[0, 1e10]])
    torch.cuda.synchronize()


def test_non_default_thresholds_ranges_and_max_dets():
    gt, dts, _ = cases.mixed_set()
    params = {'iouThrs': np.array([.3, .5, .75]), 'recThrs': np.linspace(0, 1, 11), 'maxDets': [2, 5, 20],
              'areaRng': [[0, 1e10], [0, 2000.0]], 'areaRngLbl': ['all', 'small']}
    check = dict(params)
    del check['areaRngLbl']
    r = ref.evaluate(dts, gt, 'coco', check)
    e = _run('coco', gt, dts, params)
    assert e.eval['precision'].shape == (3, 11, 5, 2, 3)
    assert np.array_equal(e.matches['ious'].cpu().numpy(), r['ious'])
    _same_after_the_ious(e, r)
    # like the reference's summarize(): the first row asks for maxDets = 100, which this run does not have
    assert (e.stats[[0, 4, 5, 10, 11]] == -1).all() and (e.stats[[1, 2, 3, 8]] > 0).all()


@pytest.mark.parametrize('T,A', [(32, 5), (7, 8), (1, 1)])
def test_problem_counts_that_need_several_passes_and_long_categories(T, A):
    """T*A beyond one wavefront (64 / T area ranges per pass, the last pass partly filled), the limits T = 32 and A = 8, and
    categories of several hundred detections: several fetches of 4 x 64 positions in the accumulator, the last one partly filled,
    with the envelope and the counts carried across them."""
    gt, dts, _ = cases.mixed_set(seed=11, n_images=6, n_cats=3, n_gt=120, n_dt=1500)
    bounds = np.linspace(0, 14400, A + 1)
    params = {'iouThrs': np.linspace(.05, .98, T) if T > 1 else np.array([.5]), 'maxDets': [1, 10, 100],
              'areaRng': [[0, 1e10]] + [[bounds[a], bounds[a + 2]] for a in range(A - 1)], 'areaRngLbl': (['all', 'small', 'medium', 'large'] + ['x'] * A)[:A]}
    check = {k: v for k, v in params.items() if k != 'areaRngLbl'}
    r = ref.evaluate(dts, gt, 'coco', check)
    assert max(np.diff(r['cat_start'])) > 512 and min(np.diff(r['cat_start'])) < 256          # the accumulator fetches 256 positions at a time
    e = _run('coco', gt, dts, params)
    assert np.array_equal(e.matches['ious'].cpu().numpy(), r['ious'])
    _same_after_the_ious(e, r)


def test_evaluator_add_equals_the_json_route():
    from mydetection_amd.api import Evaluator
    from mydetection_amd.utils.evaluation import coco
    from mydetection_amd.utils.structures import ImageObjects
    gt, dts, _ = cases.mixed_set()
    cat_ids = [1, 2, 3, 4, 5, 6]
    rng = np.random.default_rng(2)
    objects, img_ids, rows = [], [], []
    for img in range(13):                                            # one image the ground truth does not hold
        mine = [d for d in dts if d['image_id'] == 10 * (img + 1)]
        box = torch.tensor([[d['bbox'][0] + d['bbox'][2] / 2, d['bbox'][1] + d['bbox'][3] / 2, d['bbox'][2], d['bbox'][3]] for d in mine],
                           dtype=torch.float32).reshape(-1, 4) + torch.from_numpy(rng.random((len(mine), 4)).astype(np.float32)) * 0.37
        o = ImageObjects(box.cuda(), torch.tensor([d['category_id'] - 1 for d in mine], dtype=torch.int64).cuda(), None,
                         torch.tensor([d['score'] for d in mine], dtype=torch.float32).cuda(), 'cxcywh')
        objects.append(o)
        img_ids.append(10 * (img + 1))
        rows += o.to_json(10 * (img + 1), catIdx2id=cat_ids)
    ev = Evaluator(gt, 'coco', catIdx2id=cat_ids)
    ev.add(objects[:5], img_ids[:5])
    for o, i in zip(objects[5:], img_ids[5:]):
        ev.add(o, i)
    got = ev.result()
    summary, ap, ap50, ap75 = coco.coco_evaluate_bbox(rows, gt, str_print=False)
    via = coco.myCOCOeval(gt, rows, 'bbox', False)
    via.evaluate()
    via.accumulate()
    via.summarize()
    torch.cuda.synchronize()
    assert len(rows) == len(dts) and 0 < ap < 1
    assert got['summary'] == summary == via.summary and (got['stats'][0], got['stats'][1], got['stats'][2]) == (ap, ap50, ap75)
    for key in ('precision', 'recall', 'scores'):
        assert np.array_equal(got[key], via.eval[key]), key
    r = ref.evaluate(rows, gt, 'coco')
    assert np.array_equal(got['stats'], r['stats']) and np.array_equal(got['precision'], r['precision'])


def test_rotated_set_through_evaluate_json(capsys):
    from mydetection_amd.utils.evaluation import cepdof
    here = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'test_gpu_rotnms.py')).read()
    assert re.search(r'^IOU_ATOL = 1e-5$', here, re.M) and re.search(r'^MARGIN = 1e-4$', here, re.M)
    gt, dts, _ = cases.rotated_set()
    r = ref.evaluate(dts, gt, 'cepdof')
    thrs = ref.default_params()['iouThrs']
    margin = np.abs(r['ious'][:, None] - thrs[None]).min()
    print('rotated set: smallest |IoU - threshold| of the reference', margin)
    assert margin >= MARGIN, f'seed {cases.ROTATED_SEED}: a reference IoU lies within {MARGIN} of a threshold'
    summary, ap, ap50, ap75 = cepdof.evaluate_json(copy.deepcopy(dts), copy.deepcopy(gt))
    assert summary == r['summary'] and (ap, ap50, ap75) == tuple(r['stats'][:3]) and 0 < ap < ap50 < 1
    assert summary in capsys.readouterr().out
    e = _run('cepdof', gt, dts, None)
    got = e.matches['ious'].cpu().numpy()
    err = np.abs(got - r['ious']).max()
    print('rotated set: max |IoU - reference|', err)
    assert got.shape == r['ious'].shape and err <= IOU_ATOL
    _same_after_the_ious(e, r)
