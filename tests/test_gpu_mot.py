"""GPU: the track scorer's three launches (behind mydet_eval_ious_f64) against the plain restatement tests/_mot_ref.py.  Every
integer output and gt_match is compared with ==, and so is SIOU, because its order of addition is fixed.  The cases are the
smallest that reach each rule of include/mydet.h, "Scoring tracks against ground truth"."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

import _mot_cases as cases
import _mot_ref as ref

pytestmark = pytest.mark.gpu

INT_KEYS = ('counts', 'present', 'matched', 'gt_match', 'idtp', 'overlap')
TP, FP, FN, IDSW, FRAG = range(5)


def _device(rows, gt, kind, thrs, ious=None, **kw):
    from mydetection_amd import ops
    ms = ops.MotSet(ops.mot_pack(rows, gt, kind, **kw))
    given = None if ious is None else torch.tensor(ious, dtype=torch.float64, device='cuda')
    out = ops.mot_evaluate(ms, thrs, rows=True, ious=given)          # every launch's return code is checked by ops
    torch.cuda.synchronize()
    return ms.pack, {k: v.cpu().numpy() for k, v in out.items()}


def _same(got, r, exact_ious=True):
    for key in INT_KEYS:
        assert got[key].shape == r[key].shape and np.array_equal(got[key], r[key]), key
    if exact_ious:
        assert got['ious'].dtype == np.float64 and np.array_equal(got['ious'], r['ious'], equal_nan=True)
        assert got['siou'].dtype == np.float64 and np.array_equal(got['siou'], r['siou'])


def _check(scene, thrs=(0.5,), kind='coco', ious=None, n_cats=1, **kw):
    gt, rows = cases.build(scene, n_cats=n_cats)
    r = ref.evaluate(rows, gt, kind, thrs, ious=ious, **kw)
    pack, got = _device(rows, gt, kind, thrs, ious=ious, **kw)
    _same(got, r)
    return pack, got, r


def test_swap_counts_two_switches_and_the_steady_sequence_none():
    pack, got, r = _check(cases.swap())
    assert pack['S'] == 2 and got['counts'][0, 0].tolist() == [8, 0, 0, 2, 0] and got['counts'][1, 0].tolist() == [8, 0, 0, 0, 0]
    assert got['siou'][0, 0] == 8.0 and got['idtp'].ravel().tolist() == [4, 8]


def test_keep_pass_beats_the_cheaper_assignment():
    pack, got, r = _check(cases.keep_beats_cheaper())
    assert got['counts'][0, 0].tolist() == [4, 0, 0, 0, 0]
    # frame 1: rows (gt 1, gt 2) keep hypotheses (7, 8) = packed rows (2, 3), although (3, 2) has IoU 1.0 twice
    assert got['gt_match'][0].tolist() == [0, 1, 2, 3] and got['siou'][0, 0] < 3.5
    assert sorted(got['ious'][4:8].tolist()) == [0.6, 0.6, 1.0, 1.0]


def test_two_ground_truths_with_one_last_the_lower_row_wins():
    pack, got, r = _check(cases.shared_last())
    # frame 2: row 0 (gt 1) keeps hypothesis 7 (packed row 2); gt 2, whose IoU with it is 1.0, is assigned hypothesis 9: a switch
    assert got['gt_match'][0].tolist() == [0, 1, 2, 3] and got['counts'][0, 0].tolist() == [4, 0, 0, 1, 0]


def test_assignment_finds_two_matches_where_greedy_finds_one():
    pack, got, r = _check(cases.greedy_loses(), ious=cases.GREEDY_IOUS)
    assert got['counts'][0, 0, TP] == 2 and got['gt_match'][0].tolist() == [1, 0]
    assert got['siou'][0, 0] == np.float64(0.6) + np.float64(0.55)


def test_last_persists_over_unmatched_and_absent_frames():
    pack, got, r = _check(cases.persistent_last())
    assert got['counts'][0, 0].tolist() == [2, 1, 2, 1, 1] and got['present'].tolist() == [4] and got['matched'].tolist() == [[2]]


@pytest.mark.parametrize('n_rows,n_cols', [(63, 64), (64, 65), (65, 63), (130, 1024)])
def test_sizes_across_the_lane_layout_and_empty_frames(n_rows, n_cols):
    scene = cases.sizes(n_rows, n_cols, seed=n_rows)
    pack, got, r = _check(scene, thrs=(0.3, 0.6))
    c = got['counts'][0]
    assert pack['max_gt'] == n_rows and pack['max_dt'] == n_cols
    assert 0 < c[1, TP] < c[0, TP] <= 2 * min(n_rows, n_cols) and (c[:, FP] > 0).all() and (c[:, FN] > 0).all()
    assert (c[:, TP] + c[:, FN] == 2 * n_rows + 3).all() and (c[:, TP] + c[:, FP] == 2 * n_cols + 3).all()


def test_several_problems_in_one_launch():
    scene = cases.several()
    pack, got, r = _check(scene, thrs=(0.3, 0.5, 0.75), n_cats=2)
    assert (pack['S'], pack['K'], pack['U']) == (3, 2, 6) and got['counts'].shape == (6, 3, 5)
    assert (got['counts'][:, :, TP] > 0).all() and got['counts'][:, :, IDSW].sum() > 0 and got['counts'][:, :, FP].sum() > 0
    assert (got['counts'][:, 0, TP] >= got['counts'][:, 2, TP]).all() and (got['idtp'] <= got['counts'][:, :, TP]).all()
    # the same through the class, and all categories as one
    from mydetection_amd.utils.evaluation.mot import MOTeval
    gt, rows = cases.build(scene, n_cats=2)
    e = MOTeval(gt, rows, 'coco', (0.3, 0.5, 0.75), keep_rows=True)
    e.evaluate()
    result = e.summarize()
    _same(e.raw, r)
    for s in range(3):
        for t in range(3):
            units = [k * 3 + s for k in range(2)]
            ids = np.concatenate([np.arange(r['gt_id_start'][u], r['gt_id_start'][u + 1]) for u in units])
            c = r['counts'][units, t].sum(0)
            siou = np.float64(0.0) + r['siou'][units[0], t] + r['siou'][units[1], t]
            want = ref.metrics(*(int(v) for v in c), siou, int(r['idtp'][units, t].sum()), r['present'][ids].tolist(), r['matched'][t][ids].tolist())
            assert result['sequences'][s][t] == want
    assert result['overall'][1]['tp'] == int(r['counts'][:, 1, TP].sum()) and 0 < result['overall'][1]['idf1'] < 1
    assert e.summary.count('\n') == 1 + 4 * 3
    _check(scene, thrs=(0.5,), n_cats=2, use_cats=False)


def test_a_pair_exactly_at_its_threshold_is_eligible():
    half = [0.0, 0.0, 10.0, 5.0]                                     # 50 / 100: the float64 0.5 exactly
    scene = [[([(1, cases.box(0))], [(7, half)])]]
    thrs = (0.5, np.nextafter(0.5, 1.0), 1.5, -1.0)
    pack, got, r = _check(scene, thrs=thrs)
    assert got['ious'].tolist() == [0.5] and got['counts'][0, :, TP].tolist() == [1, 0, 0, 1]      # no clamp either way
    # a NaN pair value is never eligible, not even below a negative threshold
    pack, got, r = _check(scene, thrs=(-1.0, 0.5), ious=[float('nan')])
    assert got['counts'][0, :, TP].tolist() == [0, 0] and got['overlap'].sum() == 0 and got['siou'].tolist() == [[0.0, 0.0]]


def test_rotated_kind_uses_the_rotated_iou():
    thin, turned = [50.0, 50.0, 40.0, 4.0, 0.0], [50.0, 50.0, 40.0, 4.0, 90.0]
    scene = [[([(1, thin)], [(7, turned)]), ([(1, thin)], [(7, thin)])]]
    gt, rows = cases.build(scene)
    r = ref.evaluate(rows, gt, 'cepdof', [0.5])
    pack, got = _device(rows, gt, 'cepdof', [0.5])
    _same(got, r, exact_ious=False)
    assert pack['rotated'] == 1 and got['counts'][0, 0].tolist() == [1, 1, 1, 0, 0] and got['gt_match'][0].tolist() == [-1, 1]
    assert abs(got['ious'][0] - 16.0 / 304.0) < 1e-5 and abs(got['ious'][1] - 1.0) < 1e-5 and abs(r['ious'] - got['ious']).max() < 1e-5
    assert abs(got['siou'][0, 0] - got['ious'][1]) == 0
    # on columns 0-3 the first pair is one box
    assert ref.evaluate([dict(d, bbox=d['bbox'][:4]) for d in rows], {**gt, 'annotations': [dict(a, bbox=a['bbox'][:4]) for a in gt['annotations']]},
                        'coco', [0.5])['counts'][0, 0, TP] == 2


def test_identity_counts_differ_from_the_per_frame_matches():
    pack, got, r = _check(cases.id_case())
    assert got['counts'][0, 0].tolist() == [11, 0, 0, 1, 0] and got['idtp'].tolist() == [[8]]
    n = got['overlap'][0].reshape(2, 2)
    assert n.tolist() == [[3, 4], [4, 0]]
    assert got['idtp'][0, 0] == max(sum(n[o, h] for o, h in enumerate(perm)) for perm in itertools.permutations(range(2)))
    scene = cases.id_random()
    pack, got, r = _check(scene, thrs=(0.5, 0.7))
    assert (pack['max_gt_ids'], pack['max_dt_ids']) == (70, 90) and (got['idtp'] < got['counts'][:, :, TP]).all() and (got['idtp'] > 0).all()
    # more ground-truth identities than hypothesis identities: the transposed problem
    flipped = [[(hyps, gts) for gts, hyps in seq] for seq in scene]
    pack, got2, r2 = _check(flipped, thrs=(0.5, 0.7))
    assert (pack['max_gt_ids'], pack['max_dt_ids']) == (90, 70) and np.array_equal(got2['idtp'], got['idtp'])


# ---- the C ABI: errors launch nothing, and a launch writes its own outputs only ----

CANARY = 0x5A


class _Call:
    """The device buffers and structs of one scene, with every output a window of a canary-filled buffer."""

    def __init__(self, scene, thrs, n_cats=1):
        from mydetection_amd import _lib, ops
        gt, rows = cases.build(scene, n_cats=n_cats)
        self.ms = ops.MotSet(ops.mot_pack(rows, gt, 'coco'))
        self.lib, self.p = _lib.lib(), self.ms.pack
        self.thr = np.ascontiguousarray(np.asarray(thrs, np.float64))
        self.T = len(self.thr)
        self.ious = ops.eval_ious(self.ms)
        p, T = self.p, self.T
        self.sizes = {'counts': p['U'] * T * 5 * 8, 'siou': p['U'] * T * 8, 'present': p['n_gt_ids'] * 4, 'matched': T * p['n_gt_ids'] * 4,
                      'gt_match': T * p['G'] * 4, 'scratch': T * p['n_ov'] * 4, 'idtp': p['U'] * T * 8}
        self.at, total = {}, 256
        for k, n in self.sizes.items():
            self.at[k] = total
            total += (n + 255) // 256 * 256 + 256
        self.buf = torch.full((total,), CANARY, dtype=torch.uint8, device='cuda')

    def ptr(self, k):
        return ctypes.c_void_p(self.buf.data_ptr() + self.at[k])

    def window(self, k, dtype):
        return self.buf[self.at[k]:self.at[k] + self.sizes[k]].cpu().numpy().view(dtype)

    def untouched(self, written=()):
        mask = np.ones(self.buf.numel(), bool)
        for k in written:
            mask[self.at[k]:self.at[k] + self.sizes[k]] = False
        torch.cuda.synchronize()
        return bool((self.buf.cpu().numpy()[mask] == CANARY).all())

    def structs(self, **change):
        from mydetection_amd import ops
        c = ops.eval_set_struct(self.p, {k: self.ms.t[k].data_ptr() for k in ops.EVAL_SET_ARRAYS})
        m = ops.mot_set_struct(self.p, {k: self.ms.t[k].data_ptr() for k in ops.MOT_SET_ARRAYS})
        for k, v in change.items():
            setattr(c if hasattr(c, k) else m, k, v)
        return c, m

    def clear(self, c, m, **kw):
        a = dict(ious=ctypes.c_void_p(self.ious.data_ptr()), thr=ctypes.c_void_p(self.thr.ctypes.data), T=self.T, counts=self.ptr('counts'),
                 siou=self.ptr('siou'), present=self.ptr('present'), matched=self.ptr('matched'), gt_match=self.ptr('gt_match'))
        a.update(kw)
        ref_ = lambda s: ctypes.byref(s) if s is not None else None                                   # noqa: E731
        return self.lib.mydet_mot_clear_f64(ref_(c), ref_(m), a['ious'], a['thr'], a['T'], a['counts'], a['siou'], a['present'], a['matched'],
                                            a['gt_match'], None)

    def overlap(self, c, m, **kw):
        a = dict(ious=ctypes.c_void_p(self.ious.data_ptr()), thr=ctypes.c_void_p(self.thr.ctypes.data), T=self.T, scratch=self.ptr('scratch'),
                 nbytes=self.sizes['scratch'])
        a.update(kw)
        ref_ = lambda s: ctypes.byref(s) if s is not None else None                                   # noqa: E731
        return self.lib.mydet_mot_id_overlap(ref_(c), ref_(m), a['ious'], a['thr'], a['T'], a['scratch'], a['nbytes'], None)

    def assign(self, c, m, **kw):
        a = dict(T=self.T, scratch=self.ptr('scratch'), nbytes=self.sizes['scratch'], idtp=self.ptr('idtp'))
        a.update(kw)
        ref_ = lambda s: ctypes.byref(s) if s is not None else None                                   # noqa: E731
        return self.lib.mydet_mot_id_assign(ref_(c), ref_(m), a['T'], a['scratch'], a['nbytes'], a['idtp'], None)


def test_errors_launch_nothing():
    call = _Call(cases.several(), (0.3, 0.5), n_cats=2)
    p, null = call.p, ctypes.c_void_p(0)
    BADARG, UNSUPP = -1, -2
    nan = np.array([0.5, np.nan])
    nan_ptr = ctypes.c_void_p(nan.ctypes.data)
    assert p['G'] > 0 and p['D'] > 0 and p['n_pairs'] > 0 and p['n_ov'] > 0
    bad_sets = [dict(S=0), dict(S=p['I'] + 1), dict(max_gt_ids=-1), dict(n_dt_ids=-1), dict(n_ov=-1), dict(n_gt_ids=p['G'] + 1),
                dict(n_dt_ids=p['D'] + 1), dict(max_gt_ids=p['n_gt_ids'] + 1), dict(max_dt_ids=p['n_dt_ids'] + 1),
                dict(n_ov=p['n_gt_ids'] * p['n_dt_ids'] + 1), dict(seq_start=None), dict(gt_id_start=None), dict(dt_id_start=None),
                dict(ov_start=None), dict(gt_id=None), dict(dt_id=None),
                dict(rotated=2), dict(K=0), dict(G=-1), dict(dt_start=None), dict(max_gt=p['G'] + 1), dict(gt_box=None)]
    for change in bad_sets:
        c, m = call.structs(**change)
        assert call.clear(c, m) == BADARG and call.overlap(c, m) == BADARG and call.assign(c, m) == BADARG, change
    c, m = call.structs()
    for fn in (call.clear, call.overlap, call.assign):
        assert fn(None, m) == BADARG and fn(c, None) == BADARG and fn(c, m, T=0) == BADARG and fn(c, m, T=33) == UNSUPP
    for fn in (call.clear, call.overlap):
        assert fn(c, m, thr=null) == BADARG and fn(c, m, thr=nan_ptr) == BADARG and fn(c, m, ious=null) == BADARG
    for k in ('counts', 'siou', 'present', 'matched'):
        assert call.clear(c, m, **{k: null}) == BADARG, k
    assert call.overlap(c, m, nbytes=call.sizes['scratch'] - 1) == BADARG and call.overlap(c, m, scratch=null) == BADARG
    assert call.assign(c, m, nbytes=call.sizes['scratch'] - 1) == BADARG and call.assign(c, m, scratch=null) == BADARG
    assert call.assign(c, m, idtp=null) == BADARG
    assert call.lib.mydet_mot_scratch_bytes(ctypes.byref(m), call.T) == call.sizes['scratch']
    assert call.lib.mydet_mot_scratch_bytes(None, 1) == 0 and call.lib.mydet_mot_scratch_bytes(ctypes.byref(m), 33) == 0
    # counts past a cap, declared in the struct alone
    from mydetection_amd import _lib
    cap = _lib.MOT_MAX_IDS
    for change in (dict(G=3000, max_gt=1025), dict(D=3000, max_dt=1025), dict(G=3000, n_gt_ids=3000, max_gt_ids=cap + 1),
                   dict(D=3000, n_dt_ids=3000, max_dt_ids=cap + 1)):
        c, m = call.structs(**change)
        assert call.clear(c, m) == UNSUPP and call.overlap(c, m) == UNSUPP and call.assign(c, m) == UNSUPP, change
    c, m = call.structs(G=3000, max_gt=1025, S=0)                    # a bad argument is reported before a cap
    assert call.clear(c, m) == BADARG
    assert call.untouched()


def test_launches_write_their_own_outputs_only():
    thrs = (0.3, 0.5)
    scene = cases.several()
    call = _Call(scene, thrs, n_cats=2)
    gt, rows = cases.build(scene, n_cats=2)
    r = ref.evaluate(rows, gt, 'coco', thrs)
    c, m = call.structs()
    assert call.clear(c, m) == 0
    assert call.untouched(('counts', 'siou', 'present', 'matched', 'gt_match'))
    assert np.array_equal(call.window('counts', np.int64), r['counts'].ravel()) and np.array_equal(call.window('siou', np.float64), r['siou'].ravel())
    assert np.array_equal(call.window('present', np.int32), r['present']) and np.array_equal(call.window('matched', np.int32), r['matched'].ravel())
    assert np.array_equal(call.window('gt_match', np.int32), r['gt_match'].ravel())
    assert call.overlap(c, m) == 0
    assert call.untouched(('counts', 'siou', 'present', 'matched', 'gt_match', 'scratch'))
    assert np.array_equal(call.window('scratch', np.int32), r['overlap'].ravel())
    assert call.assign(c, m) == 0
    assert call.untouched(('counts', 'siou', 'present', 'matched', 'gt_match', 'scratch', 'idtp'))
    assert np.array_equal(call.window('idtp', np.int64), r['idtp'].ravel())
    # without gt_match nothing else changes
    again = _Call(scene, thrs, n_cats=2)
    c, m = again.structs()
    assert again.clear(c, m, gt_match=ctypes.c_void_p(0)) == 0 and again.untouched(('counts', 'siou', 'present', 'matched'))
    assert np.array_equal(again.window('counts', np.int64), r['counts'].ravel())


# ---- end to end ----

def _synthetic_frames(n, h, w, seed):
    from mydetection_amd import synth
    return np.stack([(synth.make_images(1, max(h, w), seed=seed + i)[0, :, :h, :w].permute(1, 2, 0).numpy() * 255).astype(np.uint8)
                     for i in range(n)])


def test_track_evaluator_on_a_tracked_detector_call():
    """A Detector with tracker= on a few synthetic frames (as tests/test_gpu_track.py makes them).  Ground truth built from the
    run's own output scores MOTA 1, IDF1 1 and no switch; with one identity relabelled halfway and one box dropped, the counts
    are the ones the edit implies."""
    from mydetection_amd import synth
    from mydetection_amd.api import Detector, TrackEvaluator, Tracker
    from mydetection_amd.models.general import name_to_model
    mdl, cfg = name_to_model('rapid')
    mdl.load_state_dict(synth.make_state_dict(mdl.state_dict(), 'rapid'), strict=True)
    det = Detector(model_and_cfg=(mdl.eval().cuda(), cfg))
    H, W, B = 150, 200, 4
    base = _synthetic_frames(1, H, W, seed=90)[0]
    frames = np.stack([base, base, np.roll(base, 3, axis=1), np.roll(base, 6, axis=1)])
    kw = dict(input_size=128, conf_thres=0.001)
    objs = det.predict_frames(frames, tracker=Tracker(min_score=0.0005), **kw)
    img_ids = [10, 11, 12, 13]
    cat_table = {c: c + 1 for c in range(100)}
    anns, rows = [], []
    for o, img in zip(objs, img_ids):
        assert o.obj_ids is not None
        for b, c, i in zip(o.bboxes.cpu().tolist(), o.cats.cpu().tolist(), o.obj_ids.cpu().tolist()):
            anns.append({'id': len(anns) + 1, 'image_id': img, 'category_id': cat_table[c], 'bbox': b, 'person_id': i})
            rows.append({'image_id': img, 'category_id': cat_table[c], 'bbox': b, 'score': 1.0, 'track_id': i})
    N = len(anns)
    assert N > B
    gt = {'images': [{'id': i} for i in img_ids], 'categories': [{'id': c} for c in sorted(set(a['category_id'] for a in anns))], 'annotations': anns}
    ev = TrackEvaluator(gt, 'cepdof', catIdx2id=cat_table)
    ev.add(objs[:2], img_ids[:2])
    for o, img in zip(objs[2:], img_ids[2:]):
        ev.add(o, img)
    res = ev.result()
    torch.cuda.synchronize()
    first = res['overall'][0]
    assert list(res['sequences']) == ['all'] and res['sequences']['all'] == res['overall']
    assert (first['tp'], first['fp'], first['fn'], first['idsw'], first['frag'], first['idtp']) == (N, 0, 0, 0, 0, N)
    assert first['mota'] == 1.0 and first['idf1'] == 1.0 and first['mt'] == first['n_ids'] and first['motp'] > 0.999
    assert 'OVERALL' in res['summary']
    # the edit: an identity that lives in all four frames becomes another one from frame 2 on; another track loses its last box
    per_id = {}
    for n, a in enumerate(rows):
        per_id.setdefault(a['track_id'], []).append(n)
    long_lived = [i for i, ns in per_id.items() if len(ns) == B]
    assert len(long_lived) >= 2, 'no two tracks live through all four frames'
    relabelled, cut = long_lived[0], long_lived[1]
    edited = [dict(a, track_id=10 ** 6) if a['track_id'] == relabelled and a['image_id'] >= 12 else a for a in rows]
    del edited[per_id[cut][-1]]
    ev.reset()
    ev.add_json(edited)
    second = ev.result()['overall'][0]
    assert (second['tp'], second['fp'], second['fn'], second['idsw'], second['frag']) == (N - 1, 0, 1, 1, 0)
    assert second['idtp'] == N - 1 - 2 and second['mota'] == 1.0 - np.float64(2) / np.float64(N)
    assert second['idf1'] == np.float64(2 * (N - 3)) / np.float64(2 * N - 1)
    # coasting output is accepted: it only adds hypotheses
    coasting = det.predict_frames(frames, tracker=Tracker(min_score=0.0005), coasting=True, **kw)
    ev.reset()
    ev.add(coasting, img_ids)
    third = ev.result()['overall'][0]
    assert third['n_hyp'] >= N and third['n_gt'] == N
    with pytest.raises(ValueError, match='obj_ids'):
        ev.add(det.predict_frames(frames, **kw), img_ids)
