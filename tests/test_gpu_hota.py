"""GPU: the three HOTA launches (behind mydet_eval_ious_f64) against the plain restatement tests/_hota_ref.py.  Every integer
output is compared with ==: pot, gt_count, dt_count, score_q, hota_match, counts, matches.  The two float64 sums are compared with
the restatement's math.fsum within rtol = max(n_terms, 1) * 2**-52: every term is >= 0, so a sum in any order is within
(n - 1) * 2**-53 of the exact one, relatively, and the tolerance is twice that bound; n_terms is counted here from the integer
arrays (the TPs, and the identity pairs with a match).  The cases are the smallest that reach each rule of include/mydet.h, "HOTA"."""
import ctypes

import numpy as np
import pytest
import torch

import _hota_ref as href
import _mot_cases as cases

pytestmark = pytest.mark.gpu

INT_KEYS = ('pot', 'gt_count', 'dt_count', 'score_q', 'hota_match', 'counts', 'matches')
TP, FN, FP = range(3)
ALPHAS19 = np.arange(1, 20) / 20.0


def _device(rows, gt, kind, alphas, ious=None, edit=None, **kw):
    from mydetection_amd import ops
    pack = ops.mot_pack(rows, gt, kind, **kw)
    ms = ops.MotSet(pack if edit is None else edit(pack))
    given = None if ious is None else torch.tensor(np.asarray(ious), dtype=torch.float64, device='cuda')
    out = ops.hota_evaluate(ms, alphas, ious=given)                  # every launch's return code is checked by ops
    torch.cuda.synchronize()
    return ms.pack, {k: v.cpu().numpy() for k, v in out.items()}


def _close(got, want, n_terms, what):
    assert got.dtype == np.float64 and got.shape == want.shape, what
    rtol = np.maximum(n_terms, 1) * 2.0 ** -52
    err = np.abs(got - want)
    print(what, 'max relative error', float((err / np.maximum(want, 1e-300)).max()) if want.size else 0.0, 'terms up to', int(np.max(n_terms, initial=0)))
    assert (err <= rtol * want).all(), what


def _same(got, r, exact_ious=True):
    for key in INT_KEYS:
        assert got[key].shape == r[key].shape and np.array_equal(got[key], r[key]), key
    if exact_ious:
        assert got['ious'].dtype == np.float64 and np.array_equal(got['ious'], r['ious'], equal_nan=True)
    n_loc = r['counts'][:, :, TP]                                     # one term per TP
    n_ass = np.array([[np.count_nonzero(r['matches'][t, r['ov_start'][u]:r['ov_start'][u + 1]]) for t in range(r['matches'].shape[0])]
                      for u in range(r['U'])]).reshape(n_loc.shape)   # one term per identity pair with a match
    assert np.array_equal(n_loc, r['n_loc']) and np.array_equal(n_ass, r['n_ass'])
    _close(got['loc_sum'], r['loc_sum'], n_loc, 'loc_sum')
    _close(got['ass_sum'], r['ass_sum'], n_ass[:, :, None], 'ass_sum')


def _check(scene, alphas=ALPHAS19, kind='coco', ious=None, n_cats=1, edit=None, unlisted=(), **kw):
    gt, rows = cases.build(scene, n_cats=n_cats)
    r = href.evaluate(rows, gt, kind, alphas, ious=ious, unlisted=unlisted, **kw)
    pack, got = _device(rows, gt, kind, alphas, ious=ious, edit=edit, **kw)
    _same(got, r)
    return pack, got, r


def test_a_single_frame():
    a, b = cases.box(0), cases.box(100)
    scene = [[([(1, a), (2, b)], [(7, cases.shifted(0.78)), (8, b), (9, cases.box(300))])]]
    for alphas in ((0.5,), ALPHAS19):                                 # T = 1 and T = 19
        pack, got, r = _check(scene, alphas=alphas)
        assert got['hota_match'].tolist() == [0, 1] and got['gt_count'].tolist() == [1, 1] and got['dt_count'].tolist() == [1, 1, 1]
        assert got['counts'].shape == (1, len(alphas), 3) and got['counts'][0, 0].tolist() == [2, 0, 1]
    assert got['counts'][0, :, TP].tolist() == [2] * 15 + [1] * 4 and got['score_q'][3] == href.Q_ONE and got['pot'][4] == href.P_ONE
    assert got['matches'].shape == (19, 6) and got['matches'][18].tolist() == [0, 0, 0, 0, 1, 0]


@pytest.mark.parametrize('n_rows,n_cols', [(9, 6), (6, 9), (65, 70)])
def test_both_orientations_the_lane_layout_and_empty_frames(n_rows, n_cols):
    """cases.sizes: a frame of n_rows x n_cols, frames without ground truth, without hypotheses and without both, and the first
    frame again with the hypotheses in another order.  65 x 70 takes more than one column per lane."""
    scene = cases.sizes(n_rows, n_cols, seed=n_rows)
    pack, got, r = _check(scene, alphas=(0.3, 0.6) if n_rows == 65 else ALPHAS19)
    c = got['counts'][0]
    assert pack['max_gt'] == n_rows and pack['max_dt'] == n_cols and np.count_nonzero(got['hota_match'] >= 0) == 2 * min(n_rows, n_cols)
    assert (c[:, TP] + c[:, FN] == 2 * n_rows + 3).all() and (c[:, TP] + c[:, FP] == 2 * n_cols + 3).all() and 0 <= c[-1, TP] < c[0, TP]
    assert got['gt_count'].max() == 3 and got['dt_count'].max() == 3 and got['score_q'].max() > 0


def test_two_sequences_two_categories_and_a_unit_without_hypothesis_identities():
    scene = cases.several(S=2, K=2)
    scene[1] = [(gts, [h for h in hyps if h[2] == 1]) for gts, hyps in scene[1]]       # sequence 1, category 2: no hypotheses at all
    pack, got, r = _check(scene, n_cats=2)
    assert (pack['S'], pack['K'], pack['U']) == (2, 2, 4) and np.diff(pack['dt_id_start']).tolist()[3] == 0 and pack['ov_start'][4] == pack['ov_start'][3]
    assert (got['counts'][:3, 0, TP] > 0).all() and got['counts'][3, :, TP].sum() == 0 and got['counts'][3, 0, FN] > 0 and got['counts'][3, 0, FP] == 0
    assert (got['ass_sum'][3] == 0).all() and (got['ass_sum'][:3, 0] > 0).all()
    # and the other way round: a unit without ground-truth identities; all categories as one
    flipped = [[(hyps, gts) for gts, hyps in seq] for seq in scene]
    pack, got, r = _check(flipped, n_cats=2, alphas=(0.5,))
    assert np.diff(pack['gt_id_start']).tolist()[3] == 0 and got['counts'][3, 0].tolist()[::2] == [0, got['counts'][3, 0, FP]]
    _check(scene, n_cats=2, alphas=(0.25, 0.5), use_cats=False)


def test_rotated_kind_scores_the_rotated_iou():
    rng = np.random.default_rng(11)
    seq = []
    for f in range(4):
        gts = [(i, [60.0 * i + 30, 50.0, 40.0, 12.0, 20.0 * i + 5 * f]) for i in range(4)]
        hyps = [(7 + i, [60.0 * i + 30 + rng.uniform(-4, 4), 50.0 + rng.uniform(-4, 4), 40.0, 12.0, 20.0 * i + 5 * f + rng.uniform(-10, 10)]) for i in range(4) if (i + f) % 4]
        seq.append((gts, hyps))
    gt, rows = cases.build([seq])
    pack, got = _device(rows, gt, 'cepdof', ALPHAS19)
    r = href.evaluate(rows, gt, 'cepdof', ALPHAS19, ious=got['ious'])    # the device's float32 rotated IoUs, tested elsewhere
    _same(got, r)
    assert pack['rotated'] == 1 and abs(href.evaluate(rows, gt, 'cepdof', ALPHAS19)['ious'] - got['ious']).max() < 1e-5
    assert got['counts'][0, 0, TP] == 12 and 0 < got['counts'][0, 13, TP] < 12 and got['counts'][0, -1, TP] == 0


def test_duplicated_boxes_take_the_lowest_column():
    a, b = cases.box(0), cases.box(2)
    # two ground truths on one box and three hypotheses on one box, then four on two with other identities: every score of a frame is equal
    scene = [[([(1, a), (2, a)], [(7, b), (8, b), (9, b)]), ([(3, a), (4, a), (5, a), (6, a)], [(10, b), (11, b)])]]
    pack, got, r = _check(scene)
    assert len(set(got['score_q'][:6].tolist())) == 1 and len(set(got['score_q'][6:].tolist())) == 1 and got['score_q'].min() > 0
    assert got['hota_match'].tolist() == [0, 1, 3, 4, -1, -1]


def test_an_unlisted_group_takes_no_part():
    scene = cases.several(S=2, K=1)
    gt, rows = cases.build(scene)
    found = {}

    def edit(pack):
        both = np.nonzero((np.diff(pack['dt_start'])[pack['groups']] > 0) & (np.diff(pack['gt_start'])[pack['groups']] > 0))[0]
        c = int(both[len(both) // 2])
        found['g'] = int(pack['groups'][c])
        sizes = np.delete(np.diff(pack['pair_start']), c)
        out = dict(pack, groups=np.delete(pack['groups'], c), pair_start=np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64))
        out['n_pairs'] = int(out['pair_start'][-1])
        return out

    pack, got = _device(rows, gt, 'coco', ALPHAS19, edit=edit)
    r = href.evaluate(rows, gt, 'coco', ALPHAS19, unlisted={found['g']})
    full = href.evaluate(rows, gt, 'coco', ALPHAS19)
    _same(got, r)
    g0, g1 = pack['gt_start'][found['g']], pack['gt_start'][found['g'] + 1]
    assert g1 > g0 and (got['hota_match'][g0:g1] == -1).all() and (full['hota_match'][g0:g1] >= 0).any()
    assert got['counts'][:, 0].sum() < full['counts'][:, 0].sum() and got['gt_count'].sum() == full['gt_count'].sum() - (g1 - g0)


def test_injected_pair_values_nan_and_exactly_at_an_alpha():
    a = cases.box(0)
    scene = [[([(1, a), (2, cases.box(50))], [(7, a), (8, cases.box(50))]), ([(1, a)], [(7, a)])]]
    nan = float('nan')
    # frame 0: [column][row]; the pair (row 1, column 1) is exactly 0.75, (row 0, column 0) exactly 0.5; frame 1: NaN
    pack, got, r = _check(scene, alphas=(0.5, np.nextafter(0.5, 1.0), 0.75, np.nextafter(0.75, 1.0)), ious=[0.5, nan, 0.0, 0.75, nan])
    assert got['counts'][0, :, TP].tolist() == [2, 1, 1, 0] and got['hota_match'].tolist() == [0, 1, 2]
    assert got['score_q'][1] == 0 and got['score_q'][4] == 0 and got['loc_sum'][0].tolist() == [1.25, 0.75, 0.75, 0.0]
    assert got['pot'].tolist() == [href.P_ONE, 0, 0, href.P_ONE] and got['gt_count'].tolist() == [2, 1] and np.isnan(got['ious'][[1, 4]]).all()
    # everything NaN: nothing aligns, every score is 0, the assignment of ties still runs and no pair reaches an alpha
    pack, got, r = _check(scene, alphas=(0.05,), ious=[nan] * 5)
    assert got['counts'][0, 0].tolist() == [0, 3, 3] and got['hota_match'].tolist() == [0, 1, 2] and not got['score_q'].any()


# ---- the caps, and the C ABI ----

def _one_frame(n):
    gts = [(i, [30.0 * (i % 32), 30.0 * (i // 32), 20.0, 20.0]) for i in range(n)]
    return cases.build([[(gts, [(5000 + i, b) for i, b in gts])]])


def test_the_largest_group_matches_the_identity_pairing():
    """1024 x 1024, injected IoUs of 0.9 on the diagonal and 0.01 elsewhere: every row and column sum is 0.9 + 1023 * 0.01, so all
    diagonal scores are one value and all others a smaller one, and the identity pairing is the only optimum (closed form; the
    numpy solver is not run at this size)."""
    from mydetection_amd import _lib
    n = _lib.EVAL_MAX_GT
    gt, rows = _one_frame(n)
    ious = np.full((n, n), 0.01)
    np.fill_diagonal(ious, 0.9)
    pack, got = _device(rows, gt, 'coco', (0.5, 0.9, np.nextafter(0.9, 1.0)), ious=ious.ravel())
    assert pack['max_gt'] == n and pack['max_dt'] == n and np.array_equal(got['hota_match'], np.arange(n))
    q = got['score_q'].reshape(n, n)
    assert len(set(np.diag(q).tolist())) == 1 and q[0, 0] > q[0, 1] >= 0 and np.count_nonzero(q == q[0, 1]) == n * n - n
    assert got['counts'][0].tolist() == [[n, 0, 0], [n, 0, 0], [0, n, n]] and (got['gt_count'] == 1).all() and (got['dt_count'] == 1).all()
    assert np.array_equal(got['matches'][1].reshape(n, n), np.eye(n, dtype=np.int32)) and not got['matches'][2].any()
    # every diagonal term of ass_sum is 1 * (1 / max(1, 1 + 1 - 1)) = 1, and every loc term 0.9
    assert got['ass_sum'][0, 1].tolist() == [float(n)] * 3 and abs(got['loc_sum'][0, 1] - 0.9 * n) <= n * 2.0 ** -52 * 0.9 * n


class _Call:
    """The structs of one scene and the raw entry points."""

    def __init__(self, scene, n_cats=1):
        from mydetection_amd import _lib, ops
        gt, rows = cases.build(scene, n_cats=n_cats)
        self.ops, self.lib = ops, _lib.lib()
        self.ms = ops.MotSet(ops.mot_pack(rows, gt, 'coco'))
        self.p = self.ms.pack
        self.out = ops.hota_evaluate(self.ms, (0.5, 0.75))
        self.alphas = np.array([0.5, 0.75])
        torch.cuda.synchronize()
        self.before = {k: v.clone() for k, v in self.out.items()}

    def structs(self, **change):
        c = self.ops.eval_set_struct(self.p, {k: self.ms.t[k].data_ptr() for k in self.ops.EVAL_SET_ARRAYS})
        m = self.ops.mot_set_struct(self.p, {k: self.ms.t[k].data_ptr() for k in self.ops.MOT_SET_ARRAYS})
        for k, v in change.items():
            setattr(c if hasattr(c, k) else m, k, v)
        return c, m

    def args(self, **kw):
        a = {k: ctypes.c_void_p(v.data_ptr()) for k, v in self.out.items()}
        a.update(alphas=ctypes.c_void_p(self.alphas.ctypes.data), T=2)
        a.update(kw)
        return a

    def align(self, c, m, **kw):
        a, ref_ = self.args(**kw), lambda s: ctypes.byref(s) if s is not None else None
        return self.lib.mydet_hota_align_f64(ref_(c), ref_(m), a['ious'], a['pot'], a['gt_count'], a['dt_count'], None)

    def match(self, c, m, **kw):
        a, ref_ = self.args(**kw), lambda s: ctypes.byref(s) if s is not None else None
        return self.lib.mydet_hota_match(ref_(c), ref_(m), a['ious'], a['pot'], a['gt_count'], a['dt_count'], a['score_q'], a['hota_match'], None)

    def score(self, c, m, **kw):
        a, ref_ = self.args(**kw), lambda s: ctypes.byref(s) if s is not None else None
        return self.lib.mydet_hota_score_f64(ref_(c), ref_(m), a['ious'], a['hota_match'], a['gt_count'], a['dt_count'], a['alphas'], a['T'],
                                             a['counts'], a['matches'], a['loc_sum'], a['ass_sum'], None)

    def untouched(self):
        torch.cuda.synchronize()
        return all(torch.equal(v, self.before[k]) or (k == 'ious' and torch.equal(v.isnan(), self.before[k].isnan())) for k, v in self.out.items())


def test_errors_launch_nothing_and_the_cap_is_unsupported():
    from mydetection_amd import _lib
    call = _Call(cases.several(), n_cats=2)
    p, null = call.p, ctypes.c_void_p(0)
    BADARG, UNSUPP = -1, -2
    assert p['G'] > 0 and p['D'] > 0 and p['n_pairs'] > 0 and p['n_ov'] > 0
    fns = (call.align, call.match, call.score)
    bad_sets = [dict(S=0), dict(S=p['I'] + 1), dict(max_gt_ids=-1), dict(n_ov=-1), dict(n_gt_ids=p['G'] + 1), dict(max_dt_ids=p['n_dt_ids'] + 1),
                dict(n_ov=p['n_gt_ids'] * p['n_dt_ids'] + 1), dict(seq_start=None), dict(gt_id_start=None), dict(dt_id_start=None),
                dict(ov_start=None), dict(gt_id=None), dict(dt_id=None), dict(rotated=2), dict(K=0), dict(G=-1), dict(dt_start=None),
                dict(max_gt=p['G'] + 1), dict(gt_box=None)]
    for change in bad_sets:
        c, m = call.structs(**change)
        assert [fn(c, m) for fn in fns] == [BADARG] * 3, change
    c, m = call.structs()
    for fn in fns:
        assert fn(None, m) == BADARG and fn(c, None) == BADARG and fn(c, m, ious=null) == BADARG and fn(c, m, gt_count=null) == BADARG
    assert call.align(c, m, pot=null) == BADARG and call.align(c, m, dt_count=null) == BADARG
    assert call.match(c, m, pot=null) == BADARG and call.match(c, m, score_q=null) == BADARG and call.match(c, m, hota_match=null) == BADARG
    for k in ('hota_match', 'dt_count', 'counts', 'matches', 'loc_sum', 'ass_sum', 'alphas'):
        assert call.score(c, m, **{k: null}) == BADARG, k
    assert call.score(c, m, T=0) == BADARG and call.score(c, m, T=33) == UNSUPP
    for bad in (0.0, -0.5, 1.0000001, float('nan')):
        alphas = np.array([0.5, bad])
        assert call.score(c, m, alphas=ctypes.c_void_p(alphas.ctypes.data)) == BADARG, bad
    # counts past a cap, declared in the struct alone: 1025 rows in a group, 1025 identities in a unit, more than 2^22 frames
    cap = _lib.MOT_MAX_IDS
    for change in (dict(G=3000, max_gt=_lib.EVAL_MAX_GT + 1), dict(D=3000, max_dt=_lib.EVAL_MAX_DT + 1), dict(G=3000, n_gt_ids=3000, max_gt_ids=cap + 1),
                   dict(D=3000, n_dt_ids=3000, max_dt_ids=cap + 1), dict(I=_lib.HOTA_MAX_FRAMES + 1, K=1)):
        c, m = call.structs(**change)
        assert [fn(c, m) for fn in fns] == [UNSUPP] * 3, change
    c, m = call.structs(G=3000, max_gt=1025, S=0)                    # a bad argument is reported before a cap
    assert call.align(c, m) == BADARG
    assert call.untouched()
    # and the launches repeat themselves bit for bit, the float sums included
    c, m = call.structs()
    assert call.align(c, m) == 0 and call.match(c, m) == 0 and call.score(c, m) == 0 and call.untouched()


# ---- end to end ----

def test_track_evaluator_with_hota_equals_moteval_on_the_same_rows():
    """A Detector with tracker= on a few synthetic frames (as tests/test_gpu_mot.py makes them), scored against ground truth built
    from the run's own output with one identity relabelled halfway and one box dropped."""
    from mydetection_amd import synth
    from mydetection_amd.api import Detector, TrackEvaluator, Tracker
    from mydetection_amd.models.general import name_to_model
    from mydetection_amd.utils.evaluation.mot import MOTeval, evaluate_json
    mdl, cfg = name_to_model('rapid')
    mdl.load_state_dict(synth.make_state_dict(mdl.state_dict(), 'rapid'), strict=True)
    det = Detector(model_and_cfg=(mdl.eval().cuda(), cfg))
    H, W = 150, 200
    base = (synth.make_images(1, max(H, W), seed=90)[0, :, :H, :W].permute(1, 2, 0).numpy() * 255).astype(np.uint8)
    frames = np.stack([base, base, np.roll(base, 3, axis=1), np.roll(base, 6, axis=1)])
    objs = det.predict_frames(frames, tracker=Tracker(min_score=0.0005), input_size=128, conf_thres=0.001)
    img_ids = [10, 11, 12, 13]
    cat_table = {c: c + 1 for c in range(100)}
    anns, rows = [], []
    for o, img in zip(objs, img_ids):
        for b, c, i in zip(o.bboxes.cpu().tolist(), o.cats.cpu().tolist(), o.obj_ids.cpu().tolist()):
            anns.append({'id': len(anns) + 1, 'image_id': img, 'category_id': cat_table[c], 'bbox': b,
                         'person_id': 10 ** 6 + i if img >= 12 and i == objs[0].obj_ids[0].item() else i})
            rows.append({'image_id': img, 'category_id': cat_table[c], 'bbox': b, 'score': 1.0, 'track_id': i})
    del anns[-1]
    gt = {'images': [{'id': i} for i in img_ids], 'categories': [{'id': c} for c in sorted(set(a['category_id'] for a in anns))], 'annotations': anns}
    ev = TrackEvaluator(gt, 'cepdof', catIdx2id=cat_table, hota=True)
    ev.add(objs, img_ids)
    res = ev.result()
    e = MOTeval(gt, rows, 'cepdof', hota=True)
    e.evaluate()
    want = e.summarize()
    torch.cuda.synchronize()
    assert res['hota'] == want['hota'] and res['summary'] == e.summary and {k: v for k, v in res.items() if k != 'summary'} == want
    h = res['hota']['overall']
    assert len(res['hota']['alphas']) == 19 and h['per_alpha']['tp'][0] == len(anns) and h['per_alpha']['fp'][0] == 1 and h['per_alpha']['fn'][0] == 0
    assert h['detre'] > 0.99 and h['loca'] > 0.999 and 0 < h['assa'] < 1 and h['hota'] < h['deta'] < 1
    # hota=False: the keys and the text of before; evaluate_json keeps its tuple
    off = TrackEvaluator(gt, 'cepdof', catIdx2id=cat_table)
    off.add(objs, img_ids)
    plain = off.result()
    assert set(plain) == {'iou_thrs', 'overall', 'sequences', 'summary'} and plain['overall'] == res['overall']
    assert res['summary'].startswith(plain['summary']) and 'hota' not in plain['summary']
    text, mota, idf1, idsw = evaluate_json(rows, gt, 'cepdof', str_print=False, hota=(0.5,))
    assert text.startswith(plain['summary']) and (mota, idf1, idsw) == tuple(plain['overall'][0][k] for k in ('mota', 'idf1', 'idsw'))
    assert evaluate_json(rows, gt, 'cepdof', str_print=False)[0] == plain['summary']
