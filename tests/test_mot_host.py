"""CPU: the track scorer's host side.  The reference assignment routine (tests/_mot_ref.assign, the restatement the GPU tests
compare the kernels with) against brute force and scipy; the packer; the summary arithmetic; the MT / ML boundaries; the
argument errors of TrackEvaluator; the declarations."""
import ctypes
import os
import re

import numpy as np
import pytest

import _mot_cases as cases
import _mot_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {'mydet_mot_clear_f64': 11, 'mydet_mot_scratch_bytes': 2, 'mydet_mot_id_overlap': 8, 'mydet_mot_id_assign': 7}


def _matrices(seed, count, max_n, max_m):
    """Random integer cost matrices; a third quantised to force ties, a third of pair costs with BIG entries."""
    rng = np.random.default_rng(seed)
    for n in range(count):
        shape = (int(rng.integers(1, max_n + 1)), int(rng.integers(1, max_m + 1)))
        if rng.random() < 0.5:
            shape = shape[::-1]
        if n % 3 == 0:
            yield rng.integers(0, 4, shape) * 100
        elif n % 3 == 1:
            iou = rng.random(shape)
            yield np.where(iou >= 0.5, ref.ONE - np.floor(iou * 65536.0).astype(np.int64), ref.BIG)
        else:
            yield rng.integers(0, 100000, shape)


def test_reference_assignment_equals_brute_force_up_to_5_by_6():
    shapes = set()
    for a in _matrices(seed=1, count=300, max_n=5, max_m=6):
        col_of_row, total = ref.assign(a)
        used = [c for c in col_of_row if c >= 0]
        assert len(used) == min(a.shape) and len(set(used)) == len(used)
        assert total == sum(int(a[r, c]) for r, c in enumerate(col_of_row) if c >= 0) == ref.brute_force(a), a
        shapes.add(a.shape)
    assert (5, 6) in shapes and (6, 5) in shapes and (1, 1) in shapes
    # the issue's 2 x 2: greedy best-first takes (0, 0) and then has no eligible partner for row 1
    cost = [[ref.pair_cost(v, 0.5)[1] for v in row] for row in ((0.9, 0.6), (0.55, 0.1))]
    assert ref.assign(cost)[0] == [1, 0]
    # a tie goes to the lowest column index
    assert ref.assign([[5, 5, 5]])[0] == [0] and ref.assign([[5, 5], [5, 5]])[0] == [0, 1]
    assert ref.pair_cost(float('nan'), 0.5) == (False, ref.BIG) and ref.pair_cost(0.5, 0.5) == (True, 32768)
    assert ref.BIG > 1024 * ref.ONE


def test_reference_assignment_equals_scipy():
    optimize = pytest.importorskip('scipy.optimize')
    for a in _matrices(seed=2, count=400, max_n=8, max_m=11):
        r, c = optimize.linear_sum_assignment(a)
        assert ref.assign(a)[1] == int(a[r, c].sum())


def test_packer_sequences_identities_and_errors():
    from mydetection_amd import ops
    scene = cases.several()
    gt, rows = cases.build(scene, n_cats=2)
    p = ops.mot_pack(rows, gt, 'coco')
    r = ref.evaluate(rows, gt, 'coco', [0.5])
    # route 1: video_id / frame_id
    assert p['seq_names'] == [0, 1, 2] and p['S'] == 3 and p['K'] == 2 and p['U'] == 6 and p['I'] == len(gt['images'])
    assert p['seq_start'].tolist() == [0, 6, 13, 21]
    for key in ('gt_id_start', 'dt_id_start', 'dt_rows', 'gt_rows'):
        assert np.array_equal(p[key], r[key]), key
    assert p['n_gt_ids'] == p['gt_id_start'][-1] and p['n_ov'] == p['ov_start'][-1] == sum(
        int(a) * int(b) for a, b in zip(np.diff(p['gt_id_start']), np.diff(p['dt_id_start'])))
    assert p['gt_id'].dtype == np.int32 and len(p['gt_id']) == p['G'] and len(p['dt_id']) == p['D']
    for u in range(p['U']):                                          # dense identities, 0 .. n - 1 inside the unit
        k, s = divmod(u, p['S'])
        lo, hi = p['gt_start'][k * p['I'] + p['seq_start'][s]], p['gt_start'][k * p['I'] + p['seq_start'][s + 1]]
        assert set(p['gt_id'][lo:hi].tolist()) == set(range(p['gt_id_start'][u + 1] - p['gt_id_start'][u]))
        assert len(p['gt_ids'][u]) == p['gt_id_start'][u + 1] - p['gt_id_start'][u]
    # route 2: no video ids -> one sequence in `images` order
    gt1, rows1 = cases.build(scene, n_cats=2, video_ids=False)
    gt1['images'] = gt1['images'][::-1]
    p1 = ops.mot_pack(rows1, gt1, 'coco')
    assert p1['seq_names'] == ['all'] and p1['seq_start'].tolist() == [0, 21] and p1['img_ids'] == [im['id'] for im in gt1['images']]
    # route 3: an explicit dict; images outside it are dropped with their rows
    seqs = {'b': [1002, 1001, 1000], 'a': [2000, 2001]}
    p2 = ops.mot_pack(rows, gt, 'coco', sequences=seqs)
    r2 = ref.evaluate(rows, gt, 'coco', [0.5], sequences=seqs)
    assert p2['seq_names'] == ['b', 'a'] and p2['img_ids'] == [1002, 1001, 1000, 2000, 2001] and p2['G'] == r2['G'] and p2['D'] == r2['D']
    assert np.array_equal(p2['gt_rows'], r2['gt_rows']) and np.array_equal(p2['dt_rows'], r2['dt_rows'])
    with pytest.raises(ValueError, match='more than one frame'):
        ops.mot_pack(rows, gt, 'coco', sequences={'a': [1000, 1001], 'b': [1001]})
    with pytest.raises(ValueError, match='not in the ground truth'):
        ops.mot_pack(rows, gt, 'coco', sequences={'a': [1000, 5]})
    # use_cats=False: one category
    p3 = ops.mot_pack(rows, gt, 'coco', use_cats=False)
    assert p3['K'] == 1 and p3['U'] == 3 and p3['G'] == len(gt['annotations']) and p3['D'] == len(rows)
    # identity keys: person_id is found; id_key overrides; none is an error
    gt4, rows4 = cases.build(scene, n_cats=2, id_key='person_id')
    assert ops.mot_id_key(gt4) == 'person_id' and ops.mot_id_key(gt) == 'track_id'
    assert np.array_equal(ops.mot_pack(rows4, gt4, 'coco')['gt_id'], p['gt_id'])
    gt5, _ = cases.build(scene, n_cats=2, id_key='who')
    assert np.array_equal(ops.mot_pack(rows, gt5, 'coco', id_key='who')['gt_id'], p['gt_id'])
    with pytest.raises(ValueError, match='identity'):
        ops.mot_pack(rows, gt5, 'coco')
    both = {**gt, 'annotations': [dict(a, person_id=0) for a in gt['annotations']]}
    assert ops.mot_id_key(both) == 'track_id'                        # the first of the two
    # a duplicate identity in a frame, on either side
    twice = rows + [dict(rows[0])]
    with pytest.raises(ValueError, match='hypothesis identity .* twice'):
        ops.mot_pack(twice, gt, 'coco')
    bad = {**gt, 'annotations': gt['annotations'] + [dict(gt['annotations'][0], id=9999)]}
    with pytest.raises(ValueError, match='ground-truth identity .* twice'):
        ops.mot_pack(rows, bad, 'coco')
    # the same identity in two categories is two identities (units are independent)
    other = rows + [dict(rows[0], category_id=3 - rows[0]['category_id'])]
    assert ops.mot_pack(other, gt, 'coco')['D'] == len(rows) + 1
    # rows without track_id, boxes of the wrong width for the kind
    with pytest.raises(ValueError, match='track_id'):
        ops.mot_pack([{k: v for k, v in rows[0].items() if k != 'track_id'}], gt, 'coco')
    with pytest.raises(ValueError, match='5-wide'):
        ops.mot_pack(rows, gt, 'cepdof')
    with pytest.raises(ValueError):
        ops.mot_pack(rows, gt, 'segm')


def test_summary_arithmetic_from_hand_written_counts():
    from mydetection_amd import ops
    m = ops.mot_metrics(tp=8, fp=3, fn=2, idsw=1, frag=2, siou=6.0, idtp=7, present=[5, 5], matched=[5, 3])
    assert (m['n_gt'], m['n_hyp'], m['idfp'], m['idfn']) == (10, 11, 4, 3)
    assert m['mota'] == 1.0 - np.float64(6) / np.float64(10) and m['motp'] == 0.75
    assert m['precision'] == np.float64(8) / np.float64(11) and m['recall'] == 0.8
    assert m['idf1'] == np.float64(14) / np.float64(21) and m['idp'] == np.float64(7) / np.float64(11) and m['idr'] == 0.7
    assert (m['n_ids'], m['mt'], m['pt'], m['ml'], m['frag'], m['idsw']) == (2, 1, 1, 0, 2, 1)
    assert m == ref.metrics(8, 3, 2, 1, 2, 6.0, 7, [5, 5], [5, 3])
    empty = ops.mot_metrics(0, 0, 0, 0, 0, 0.0, 0, [], [])
    assert all(np.isnan(empty[k]) for k in ('mota', 'motp', 'precision', 'recall', 'idf1', 'idp', 'idr')) and empty['n_ids'] == 0
    # per sequence and overall from raw arrays: S = 2, K = 1, T = 1
    pack = {'S': 2, 'K': 1, 'seq_names': ['a', 'b'], 'gt_id_start': np.array([0, 1, 3])}
    raw = {'counts': np.array([[[4, 1, 0, 0, 0]], [[4, 2, 2, 1, 2]]]), 'siou': np.array([[3.0], [3.0]]), 'idtp': np.array([[4], [3]]),
           'present': np.array([4, 5, 1]), 'matched': np.array([[4, 3, 1]])}
    result, text = ops.mot_summarize(raw, pack, np.array([0.5]))
    assert result['sequences']['a'][0] == ops.mot_metrics(4, 1, 0, 0, 0, 3.0, 4, [4], [4])
    assert result['sequences']['b'][0] == ops.mot_metrics(4, 2, 2, 1, 2, 3.0, 3, [5, 1], [3, 1])
    assert result['overall'][0] == ops.mot_metrics(8, 3, 2, 1, 2, 6.0, 7, [4, 5, 1], [4, 3, 1]) and result['iou_thrs'] == [0.5]
    lines = text.splitlines()
    assert len(lines) == 4 and lines[0].split()[:4] == ['sequence', 'IoU', 'mota', 'motp'] and lines[3].split()[0] == 'OVERALL'
    assert lines[3].split()[2] == '0.4000' and lines[1].split()[0] == 'a'


def test_mostly_tracked_and_mostly_lost_boundaries():
    from mydetection_amd import ops

    def classes(present, matched):
        m = ops.mot_metrics(0, 0, 0, 0, 0, 0.0, 0, present, matched)
        return m['mt'], m['pt'], m['ml']
    assert classes([5], [4]) == (1, 0, 0)                            # exactly 4 of 5 frames: mostly tracked
    assert classes([5], [1]) == (0, 1, 0)                            # exactly 1 of 5 frames: not mostly lost
    assert classes([5], [0]) == (0, 0, 1)
    assert classes([10], [7]) == (0, 1, 0) and classes([10], [8]) == (1, 0, 0) and classes([10], [1]) == (0, 0, 1) and classes([10], [2]) == (0, 1, 0)
    assert classes([5, 5, 5, 1], [5, 3, 0, 1]) == (2, 1, 1)


def test_track_evaluator_argument_errors():
    torch = pytest.importorskip('torch')
    from mydetection_amd.api import TrackEvaluator
    from mydetection_amd.utils.structures import ImageObjects
    gt, rows = cases.build(cases.swap())
    with pytest.raises(ValueError, match='kind'):
        TrackEvaluator(gt, 'segm')
    with pytest.raises(ValueError, match='thresholds'):
        TrackEvaluator(gt, 'coco', iou_thrs=())
    with pytest.raises(ValueError, match='thresholds'):
        TrackEvaluator(gt, 'coco', iou_thrs=[0.5, float('nan')])
    with pytest.raises(ValueError, match='thresholds'):
        TrackEvaluator(gt, 'coco', iou_thrs=np.linspace(0, 1, 33))
    with pytest.raises(ValueError, match='sequences'):
        TrackEvaluator(gt, 'coco', sequences=[[1000, 1001]])
    with pytest.raises(ValueError, match='not in the ground truth'):
        TrackEvaluator(gt, 'coco', sequences={'a': [1]})
    with pytest.raises(ValueError, match='identity'):
        TrackEvaluator(gt, 'coco', id_key='person_id')
    ev = TrackEvaluator(gt, 'coco', catIdx2id=[1])
    boxes, cats, scores = torch.tensor([[5.0, 5.0, 10.0, 10.0]]), torch.zeros(1, dtype=torch.int64), torch.ones(1)
    with pytest.raises(ValueError, match='obj_ids'):
        ev.add(ImageObjects(boxes, cats, None, scores, 'cxcywh'), 1000)
    rot = ImageObjects(torch.tensor([[5.0, 5.0, 10.0, 10.0, 0.0]]), cats, None, scores, 'cxcywhd', obj_ids=torch.tensor([3]))
    with pytest.raises(ValueError, match='cxcywh boxes'):
        ev.add(rot, 1000)
    good = ImageObjects(boxes, cats, None, scores, 'cxcywh', obj_ids=torch.tensor([3]))
    with pytest.raises(ValueError, match='2 ImageObjects and 1 image ids'):
        ev.add([good, good], [1000])
    with pytest.raises(ValueError, match='obj_ids'):                 # nothing is added unless everything can be
        ev.add([good, ImageObjects(boxes, cats, None, scores, 'cxcywh')], [1000, 1001])
    assert len(ev) == 0
    ev.add(good, 1000)
    ev.add_json(rows[:2])
    c = ev.columns()
    assert len(ev) == 3 and c['track_id'] == [3, 7, 8] and c['bbox'].shape == (3, 4) and c['bbox'][0].tolist() == [0.0, 0.0, 10.0, 10.0]
    with pytest.raises(ValueError, match='track_id'):
        ev.add_json([{'image_id': 1000, 'category_id': 1, 'bbox': [0, 0, 1, 1], 'score': 1.0}])
    ev.reset()
    assert len(ev) == 0
    with pytest.raises(ValueError, match='cxcywhd boxes'):
        TrackEvaluator(gt, 'cepdof').add(good, 1000)


def test_entry_points_are_declared_exported_bound_and_documented():
    from mydetection_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'mydet.h')).read()
    dll = ctypes.CDLL(_lib.LIB_PATH)
    for name, nargs in NAMES.items():
        assert re.search(r'\bint(64_t)?\s+' + name + r'\s*\(', header)
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name]) == nargs
        assert hasattr(dll, name) and getattr(_lib.lib(), name).argtypes == _lib.SIGNATURES[name]
    assert 'mydet_mot_scratch_bytes' in _lib.RETURNS_I64
    assert re.search(r'#define\s+MYDET_MOT_MAX_IDS\s+' + str(_lib.MOT_MAX_IDS) + r'\b', header) and _lib.MOT_MAX_IDS == 1024
    assert 'typedef struct mydet_mot_set' in header
    s = _lib.MotSet
    assert ctypes.sizeof(s) == 88 and s.n_gt_ids.offset == 16 and s.n_ov.offset == 32 and s.seq_start.offset == 40 and s.ov_start.offset == 80
    design = open(os.path.join(ROOT, 'DESIGN.md')).read()
    readme = open(os.path.join(ROOT, 'README.md')).read()
    for text in ('floor(iou * 65536.0)', '1 << 27', 'u = k*S + s', 'lowest column index', '5 * matched >= 4 * present'):
        assert text in header + design and text in design, text
    for text in ('TrackEvaluator', 'HOTA', 'TrackEval', 'motp'):
        assert text in readme, text
    mk = open(os.path.join(ROOT, 'mydetection_amd', 'csrc', 'Makefile')).read()
    assert re.search(r'SRCS_EXACT\s*=.*\bmot\.hip\b', mk)
    from mydetection_amd.api import TrackEvaluator                                 # noqa: F401
    from mydetection_amd.utils.evaluation import mot
    assert callable(mot.evaluate_json) and callable(mot.MOTeval)
    assert (ref.ONE, ref.BIG) == (65536, 1 << 27)
