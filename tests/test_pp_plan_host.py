"""CPU: the host restatement of postprocess_kernel's launch rules (tests/_pp_plan.py) against oracle.postprocess, and the
claims of every case of tests/test_gpu_postprocess_branches.py (tests/_pp_cases.py).  No GPU."""
import numpy as np
import pytest

import _pp_cases as cases
import _pp_plan as plan
from oracle import postprocess as pp

F32 = np.float32


def _oracle_selected(scores, conf, topk=512):
    """The candidates oracle.postprocess.post_process selects before its NMS, restated from its first four lines."""
    sel = np.nonzero(scores >= F32(conf))[0]
    if len(sel) > topk:
        sel = sel[np.argsort(-scores[sel], kind='stable')[:topk]]
    return np.sort(sel)


def _oracle_selected_through_post_process(scores, conf, topk=512):
    """The same set read from post_process itself: boxes that never overlap and one class each, so the NMS keeps everything."""
    N = len(scores)
    b = np.zeros((N, 4), F32)
    b[:, 0] = 10 * (np.arange(N) % 1000)
    b[:, 1] = 10 * (np.arange(N) // 1000)
    b[:, 2:] = 4
    return np.sort(pp.post_process(b, np.zeros(N, np.int64), scores, conf, 0.5, topk)[3])


def _score_sets():
    rng = np.random.Generator(np.random.PCG64(5))
    N = 5000
    u = rng.random(N, dtype=F32)
    yield 'random', u, 0.3
    yield 'random_all_pass', u, 0.0
    yield 'ties_1/64', np.round(u * 64) / F32(64), 0.25
    yield 'ties_1/4', np.round(u * 4) / F32(4), 0.25
    yield 'all_equal', np.full(N, 0.5, F32), 0.5
    yield 'negative', -u, -np.inf
    yield 'negative_ties', -np.round(u * 16) / F32(16) - F32(0.125), -np.inf
    yield 'mixed', (u - F32(0.8)).astype(F32), -0.5
    yield 'subnormal', rng.integers(1, 1 << 23, N).astype(np.uint32).view(F32), 0.0
    yield 'with_inf', np.where(u > 0.95, F32(np.inf), np.where(u < 0.05, F32(-np.inf), u)).astype(F32), -np.inf
    yield 'with_nan', np.where(u > 0.6, F32(np.nan), u).astype(F32), 0.1
    yield 'few', np.where(u > 0.99, u, F32(0)).astype(F32), 0.5


@pytest.mark.parametrize('name,scores,conf', list(_score_sets()), ids=[s[0] for s in _score_sets()])
@pytest.mark.parametrize('topk', [512, 65, 1])
def test_largest_keys_are_the_oracles_selection(name, scores, conf, topk):
    """The `topk` largest keys are the oracle's set, the plan's k-th key cuts off exactly them, and the key order is the
    oracle's order (score descending, index ascending)."""
    k = plan.keys(scores, conf)
    want = _oracle_selected(scores, conf, topk)
    np.testing.assert_array_equal(np.sort(plan.key_index(np.sort(k)[::-1][:topk])), want)
    np.testing.assert_array_equal(plan.selected(scores, conf, topk), want)
    if topk == 512:
        np.testing.assert_array_equal(want, _oracle_selected_through_post_process(scores, conf))
    passing = plan.passing(scores, conf)
    np.testing.assert_array_equal(plan.key_index(np.sort(k)[::-1]), passing[np.argsort(-scores[passing], kind='stable')])
    p = plan.topk_plan(scores, conf, topk)
    assert p.n == len(passing) and (p.levels == 0) == (p.n <= topk)
    if p.levels:
        assert int((k >= np.uint64(p.kth)).sum()) == topk


def test_keys_make_one_score_of_the_two_zeros():
    """Left out of the sets above: -0.0 and +0.0.  The restated sortable() gives both one key, as the kernel's does, so the
    index decides between them and the selection is the oracle's indices 0..511."""
    s = np.zeros(800, F32)
    s[1::2] = -0.0
    assert np.signbit(s).sum() == 400 and len(set(plan.sortable(s).tolist())) == 1
    np.testing.assert_array_equal(plan.selected(s, 0.0), np.arange(512))
    np.testing.assert_array_equal(_oracle_selected_through_post_process(s, 0.0), np.arange(512))
    assert plan.sortable(np.array([-1e-45], F32))[0] < plan.sortable(np.array([0.0], F32))[0] < plan.sortable(np.array([1e-45], F32))[0]


def test_sortable_is_monotone():
    v = np.array([-np.inf, -3.0, -1.0, -1e-38, -1e-45, 0.0, 1e-45, 1e-38, 0.5, 1.0, np.inf], F32)
    k = plan.sortable(v).astype(np.int64)
    assert (np.diff(k) > 0).all()


def _chain_mask(links):
    m = np.zeros((links + 1, links + 1), bool)
    m[np.arange(links), np.arange(links) + 1] = True
    return m


def test_rounds_needed_on_chains_and_the_hand_over_length():
    """rounds_needed is L + 1 for a chain of L links (derivation: tests/_pp_plan.py), so with MAX_ROUNDS = 12 the last chain
    that settles has 11 links; group D of the GPU test is built around the lengths found here."""
    for L in range(0, 40):
        assert plan.rounds_needed(_chain_mask(L)) == L + 1
    settled = [L for L in range(0, 40) if plan.rounds_needed(_chain_mask(L)) <= plan.MAX_ROUNDS]
    L0 = max(settled)
    assert settled == list(range(L0 + 1)) and L0 == 11
    assert plan.rounds_needed(_chain_mask(L0)) == 12 and plan.rounds_needed(_chain_mask(L0 + 1)) == 13
    names = {img['name'] for img in cases.launches()['D_handover']['images']}
    assert names == {f'chain_{L}_links_nsel_{n}' for L in (L0 - 1, L0, L0 + 1, L0 + 2) for n in (65, 200, 512)}
    # other shapes: a box suppressing everything settles in two rounds, two chains side by side in the longer one's count
    star = np.zeros((30, 30), bool)
    star[0, 1:] = True
    assert plan.rounds_needed(star) == 2
    both = np.zeros((12, 12), bool)
    both[:5, :5], both[5:, 5:] = _chain_mask(4), _chain_mask(6)
    assert plan.rounds_needed(both) == 7


@pytest.mark.parametrize('seed', range(6))
def test_fixed_point_is_the_greedy_nms(seed):
    """The kept set read from the settled `removed` is nms_single_class's, on random boxes dense enough for long dependency chains."""
    rng = np.random.Generator(np.random.PCG64(100 + seed))
    n = 300
    b = np.empty((n, 4), F32)
    b[:, :2] = rng.random((n, 2), dtype=F32) * (40 + 30 * seed)
    b[:, 2:] = rng.random((n, 2), dtype=F32) * 20 + 1
    s = rng.random(n, dtype=F32)
    if seed % 2:
        s = np.round(s * 8) / F32(8)                    # score ties: the index decides
    c = np.zeros(n, np.int64)
    thr = (0.1, 0.3, 0.5)[seed % 3]
    order, mask = plan.order_and_mask(b, c, s, np.arange(n), thr)
    assert not np.tril(mask).any()
    kept = order[plan.greedy_from_rounds(mask)]
    np.testing.assert_array_equal(kept, pp.nms_single_class(pp.cxcywh_to_x1y1x2y2(b), s, thr))
    assert plan.rounds_needed(mask) >= 2


def test_order_and_mask_over_classes_is_post_process():
    rng = np.random.Generator(np.random.PCG64(9))
    n = 400
    b = np.empty((n, 4), F32)
    b[:, :2] = rng.random((n, 2), dtype=F32) * 60
    b[:, 2:] = rng.random((n, 2), dtype=F32) * 20 + 1
    s = rng.random(n, dtype=F32)
    c = rng.integers(0, 4, n).astype(np.int64)
    order, mask = plan.order_and_mask(b, c, s, plan.selected(s, 0.2), 0.3)
    np.testing.assert_array_equal(order[plan.greedy_from_rounds(mask)], pp.post_process(b, c, s, 0.2, 0.3)[3])


def test_case_names_are_complete():
    assert sorted(cases.launches()) == sorted(cases.NAMES)


@pytest.mark.parametrize('name', cases.NAMES)
def test_every_case_takes_the_plan_it_claims(name):
    L = cases.launches()[name]
    plans = cases.check_claims(L)
    N = {len(img['s']) for img in L['images']}
    assert len(N) == 1 and N.pop() <= 200000
    assert len(plans) == len(L['images'])                # image names are unique inside a launch


@pytest.mark.parametrize('topk', cases.B_TOPKS)
def test_every_topk_case_takes_the_plan_it_claims(topk):
    L = cases.b_launch(topk)
    plans = cases.check_claims(L, topk)
    assert plans['n_1500'].need <= topk and plans['n_1500'].levels >= 1 and plans['n_is_topk'].levels == 0
    for img in L['images']:                                 # the plan's selection at this topk is the oracle's
        np.testing.assert_array_equal(plan.selected(img['s'], L['conf'], topk), _oracle_selected(img['s'], L['conf'], topk))


def test_groups_cover_what_they_name():
    """The coverage the table of test_gpu_postprocess_branches.py promises, counted over all cases."""
    L = cases.launches()
    plans = {}
    for n in ('A_topk', 'A4_N200000', 'A_N16384', 'A_N16385', 'C_negative'):
        for img in L[n]['images']:
            plans[n, img['name']] = plan.topk_plan(img['s'], L[n]['conf'])
    assert {p.levels for p in plans.values()} == {0, 1, 2, 3, 4, 5}
    assert any(p.levels == 1 and p.bins[-1] == plan.LIST for p in plans.values())
    assert any(p.levels == 5 and p.bins[0] == plan.LIST + 1 for p in plans.values())
    assert any(p.levels and p.need == 1 and p.list_len > 1 for p in plans.values())
    assert any(p.levels and p.need == p.list_len > 1 for p in plans.values())
    assert {p.tail_trips for p in plans.values()} == {0, 1, 2}
    assert {p.sweeps for p in plans.values()} >= {1, 2, 13}
    assert {p.n for p in plans.values()} >= {0, 512, 513, 16384, 16385, 24577}
    rounds = {img['claim']['rounds'] for img in L['D_handover']['images']}
    assert rounds == {11, 12, 13, 14}
    # a pair on the threshold is kept, one just above it is not
    for name, v in cases.E_IOU.items():
        assert name not in cases.e_suppressed(v) and name in cases.e_suppressed(float(np.nextafter(v, 0.0)))
    assert cases.e_suppressed(cases.F45) >= {'iou_4508/10000'} and 'iou_4488/10000' not in cases.e_suppressed(cases.F45)
    # the float32 quotient of the 45/100 pair is float32(0.45) itself, and the oracle's IoU of every dyadic pair is exact
    img = cases.e_image()
    _, mask = plan.order_and_mask(img['b'], img['c'], img['s'], np.arange(len(img['s'])), float(np.nextafter(cases.F45, 0.0)))
    names = list(cases.E_PAIRS)
    assert {names[i // 2] for i, j in zip(*np.nonzero(mask))} == cases.e_suppressed(float(np.nextafter(cases.F45, 0.0)))
