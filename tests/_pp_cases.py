"""Inputs of tests/test_gpu_postprocess_branches.py, with the path each one claims to take.  Numpy only, no GPU.

A launch is  dict(name, conf, thr, images)  and an image  dict(name, b [N,4], c [N], s [N], claim).  A claim names fields of
_pp_plan.Plan with the values the image must give (n, sweeps, levels, bins, need, tail, tail_trips), `rounds` (the count of
_pp_plan.rounds_needed on the image's suppression matrix; the kernel settles iff rounds <= 12) with `nsel`, and `bad` (a selected
class id outside [0, 4096): count -1).  check_claims() asserts them; tests/test_pp_plan_host.py runs it on every launch, so a
wrong claim fails without a GPU, and the GPU test runs it again before each launch.

Boxes.  Outside groups D and E candidate i lies on a grid: cell = i // 2, a 4 x 4 box at (16 * (cell % 512) + (i & 1),
16 * (cell // 512)), class cell % 5.  The two candidates of a cell overlap with IoU 12 / 20 = 0.6 and nothing else overlaps, so
at thr = 0.45 every pair test is decided far from the threshold, and a wrongly selected or wrongly ordered candidate changes
which one of a cell survives.  Group D's chains are 20 x 20 boxes 12 apart (IoU 0.25 with the neighbour, 0 beyond) at thr = 0.2."""
import numpy as np

import _pp_plan as plan

F32 = np.float32
CONF, THR = 0.25, 0.45


def grid(N, classes=5):
    i = np.arange(N)
    cell = i // 2
    b = np.zeros((N, 4), F32)
    b[:, 0] = 16 * (cell % 512) + (i & 1)
    b[:, 1] = 16 * (cell // 512)
    b[:, 2:] = 4
    return b, (cell % classes).astype(np.int64)


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def _below(N, rng):
    """Scores that fail CONF."""
    return (rng.random(N, dtype=F32) * F32(0.2)).astype(F32)


def _distinct(k, rng, lo=0.3, hi=1.0):
    """k distinct float32 scores in (lo, hi), shuffled: evenly spaced, far more than an ulp apart."""
    return (lo + (hi - lo) * (rng.permutation(k) + 0.5) / k).astype(F32)


def _above(k):
    """k distinct scores in [0.75, 0.875): above a tie at 0.5, and in other level-0 bins than it."""
    assert k <= 512
    return (0.75 + np.arange(k) / 4096.0).astype(F32)


def _image(name, N, seed, fill, claim, classes=5):
    """fill(s, rng, pick) writes the passing scores into s; pick(k) draws k unused indices."""
    rng = _rng(seed)
    s = _below(N, rng)
    free = rng.permutation(N)
    used = [0]

    def pick(k):
        out = np.sort(free[used[0]:used[0] + k])
        used[0] += k
        assert len(out) == k
        return out
    fill(s, rng, pick)
    b, c = grid(N, classes)
    return dict(name=name, b=b, c=c, s=s, claim=claim)


# ------------------------------------------------------------------------------------------------------------- A. top-k selection
def _a_images(N):
    def a0(s, rng, pick):
        s[pick(512)] = _distinct(512, rng)

    def a1_tie(s, rng, pick):
        s[pick(513)] = 0.5

    def a1_two(s, rng, pick):
        s[pick(512)] = 0.75
        s[pick(1)] = 0.5

    def a2(s, rng, pick):
        s[pick(20000)] = _distinct(20000, rng)

    def a3(s, rng, pick):
        s[pick(2048)] = (np.full(2048, 0.5, F32).view(np.uint32) + rng.permutation(2048).astype(np.uint32) // 8).view(F32)
        s[pick(300)] = _above(300)

    def a5(s, rng, pick):
        s[5000:8000] = 0.5
        free = np.setdiff1d(np.arange(N), np.arange(5000, 8000))
        s[rng.choice(free, 300, replace=False)] = _above(300)

    def a6(s, rng, pick):
        s[:] = 0.5

    def empty(s, rng, pick):
        pass

    def few(s, rng, pick):
        s[pick(100)] = _distinct(100, rng)

    def list1024(s, rng, pick):
        s[pick(1024)] = 0.5
        s[pick(100)] = _above(100)

    def list1025(s, rng, pick):
        s[pick(1025)] = 0.5
        s[pick(100)] = _above(100)

    def need_one(s, rng, pick):
        s[pick(700)] = 0.5
        s[pick(511)] = _above(511)

    def need_all(s, rng, pick):
        s[pick(300)] = 0.5
        s[pick(212)] = _above(212)
        s[pick(1000)] = 0.3

    def passing(k):
        def f(s, rng, pick):
            s[pick(k)] = _distinct(k, rng)
        return f

    return [
        _image('A0_512_pass', N, 1, a0, dict(n=512, levels=0, tail=False)),
        _image('A1_513_tied', N, 2, a1_tie, dict(n=513, levels=1, bins=(513,), need=512)),
        _image('A1_513_two_scores', N, 3, a1_two, dict(n=513, levels=1, bins=(512,), need=512)),
        _image('A2_20000_distinct', N, 4, a2, dict(n=20000, levels=2, tail=True, tail_trips=1)),
        _image('A3_ulps', N, 5, a3, dict(n=2348, levels=3, bins=(2048, 2048, 8), need=4)),
        _image('A5_3000_contiguous', N, 6, a5, dict(n=3300, levels=5, bins=(3000, 3000, 3000, 3000, 16), need=12)),
        _image('A6_all_equal', N, 7, a6, dict(n=N, levels=5, bins=(N, N, N, N, 16), need=16, tail=True, tail_trips=2)),
        _image('empty', N, 8, empty, dict(n=0, levels=0)),
        _image('few_100', N, 9, few, dict(n=100, levels=0)),
        _image('LIST_1024', N, 10, list1024, dict(n=1124, levels=1, bins=(1024,), need=412)),
        _image('LIST_1025', N, 11, list1025, dict(n=1125, levels=5, bins4=(1025, 1025, 1025, 1025))),
        _image('need_1', N, 12, need_one, dict(n=1211, levels=1, bins=(700,), need=1)),
        _image('need_whole_bin', N, 13, need_all, dict(n=1512, levels=1, bins=(300,), need=300)),
        _image('n_16384', N, 14, passing(16384), dict(n=16384, levels=2, tail=False, tail_trips=0)),
        _image('n_16385', N, 15, passing(16385), dict(n=16385, levels=2, tail=True, tail_trips=1)),
        _image('n_24577', N, 16, passing(24577), dict(n=24577, levels=2, tail=True, tail_trips=2)),
    ]


def _a4_images(N):
    def a4(s, rng, pick):
        tied = np.arange(0, N, 100)
        s[tied] = 0.5
        free = np.setdiff1d(np.arange(N), tied)
        s[rng.choice(free, 300, replace=False)] = _above(300)

    def five(s, rng, pick):                      # 3000 contiguous ties across index 65536: level 3 splits them 1536 / 1464
        s[64000:67000] = 0.5
        free = np.setdiff1d(np.arange(N), np.arange(64000, 67000))
        s[rng.choice(free, 300, replace=False)] = _above(300)

    def empty(s, rng, pick):
        pass

    def few(s, rng, pick):
        s[pick(37)] = _distinct(37, rng)

    return [
        _image('A4_every_100th', N, 21, a4, dict(n=2300, levels=4, bins=(2000, 2000, 2000, 656), need=212, sweeps=13)),
        _image('five_levels_across_65536', N, 22, five, dict(n=3300, levels=5, bins=(3000, 3000, 3000, 1536, 16), need=4)),
        _image('empty', N, 23, empty, dict(n=0, levels=0)),
        _image('few_37', N, 24, few, dict(n=37, levels=0)),
    ]


def _all_pass(N):
    def distinct(s, rng, pick):
        s[:] = _distinct(N, rng)

    def equal(s, rng, pick):
        s[:] = 0.5
    sw, tail = -(-N // 16384), N > 16384
    return [_image(f'N{N}_distinct', N, 30 + N % 7, distinct, dict(n=N, sweeps=sw, levels=2, tail=tail, tail_trips=int(tail))),
            _image(f'N{N}_equal', N, 31 + N % 7, equal, dict(n=N, sweeps=sw, levels=5, bins=(N, N, N, N, 16), need=16, tail=tail))]


# ----------------------------------------------------------------------------------------------------------------- C. score values
def _c_launches():
    N = 3000
    out = []

    def neg(s, rng, pick):
        s[:] = -_distinct(N, rng, 0.0, 1.0)
        s[17] = -np.inf

    def neg_tie(s, rng, pick):
        s[:] = -0.5

    out.append(dict(name='C_negative', conf=-np.inf, thr=THR, images=[
        _image('all_negative', N, 40, neg, dict(n=N, levels=1)),
        _image('all_minus_half', N, 41, neg_tie, dict(n=N, levels=5, bins=(N, N, N, N, 16), need=16))]))

    def mixed(s, rng, pick):                      # 391 positive, 1043 pass -0.25: the boundary lies among the negative ones
        s[:] = (-1.0 + 1.15 * (rng.permutation(N) + 0.5) / N).astype(F32)
    out.append(dict(name='C_mixed_signs', conf=-0.25, thr=THR, images=[_image('mixed', N, 42, mixed, dict(n=1043, levels=1))]))

    tiny = float(np.uint32(1).view(F32))          # the smallest subnormal, 2^-149

    def subnormal(s, rng, pick):                  # k * 2^-149, k = 0 .. N-1, shuffled: +0 and 2999 subnormals
        s[:] = rng.permutation(N).astype(np.uint32).view(F32)
    out.append(dict(name='C_subnormal_conf0', conf=0.0, thr=THR, images=[_image('subnormal', N, 43, subnormal, dict(n=N, levels=2))]))
    out.append(dict(name='C_subnormal_conf_tiny', conf=tiny, thr=THR,
                    images=[_image('subnormal', N, 43, subnormal, dict(n=N - 1, levels=2))]))

    def inf(s, rng, pick):
        s[pick(600)] = np.inf
        s[pick(900)] = _distinct(900, rng)

    def inf_few(s, rng, pick):
        s[pick(40)] = np.inf
        s[pick(900)] = _distinct(900, rng)
    out.append(dict(name='C_inf', conf=CONF, thr=THR, images=[
        _image('inf_600', N, 44, inf, dict(n=1500, levels=1, bins=(600,), need=512)),
        _image('inf_40', N, 45, inf_few, dict(n=940, levels=1))]))

    def nan(s, rng, pick):
        s[:] = _distinct(N, rng, -1.0, 1.0)
        s[pick(700)] = np.uint32(0x7FC00000).view(F32)
        s[pick(700)] = np.uint32(0xFFC00000).view(F32)
        s[pick(100)] = np.uint32(0x7F800001).view(F32)       # a signalling NaN just behind +inf
    for conf, tag in ((-np.inf, '-inf'), (0.25, '0.25'), (np.nan, 'nan')):
        img = _image('nan', N, 46, nan, dict(n=0, levels=0) if conf != conf else dict(n=1500) if conf < 0 else dict())
        out.append(dict(name=f'C_nan_conf_{tag}', conf=conf, thr=THR, images=[img]))

    # signed zero.  Across the top-k boundary: s[i] = +0 for even i, -0 for odd i, conf = 0; the oracle takes indices 0..511.
    def zeros(first):
        def f(s, rng, pick):
            s[:] = 0.0
            s[first::2] = -0.0
        return f
    out.append(dict(name='C_signed_zero_boundary', conf=0.0, thr=THR, images=[
        _image('plus_minus', 800, 47, zeros(1), dict(n=800, levels=1, bins=(800,), need=512)),
        _image('minus_plus', 800, 48, zeros(0), dict(n=800, levels=1, bins=(800,), need=512))]))

    # n <= topk: the two candidates of a cell are (+0, -0) in even cells and (-0, +0) in odd ones; the lower index must win both
    def zero_pairs(s, rng, pick):
        s[:] = 0.0
        cell = np.arange(len(s)) // 2
        s[(np.arange(len(s)) & 1) == (1 - cell % 2)] = -0.0
    out.append(dict(name='C_signed_zero_pairs', conf=0.0, thr=THR, images=[_image('pairs', 400, 49, zero_pairs, dict(n=400, levels=0))]))
    return out


# ------------------------------------------------------------------------------------------------------ B. topk below 512 (dense)
B_TOPKS = (1, 2, 63, 64, 65, 511)


def b_launch(topk):
    """Three images for a run-time topk: 1500 distinct scores pass (the search runs with need = topk), topk // 2 pass (rows from
    the count to topk are zero-filled), exactly topk pass (the last n that skips the search)."""
    N = 2000

    def passing(k):
        def f(s, rng, pick):
            s[pick(k)] = _distinct(k, rng)
        return f
    return dict(name=f'B_topk_{topk}', conf=CONF, thr=THR, images=[
        _image('n_1500', N, 50, passing(1500), dict(n=1500, levels=1)),
        _image('n_half_topk', N, 51, passing(topk // 2), dict(n=topk // 2, levels=0)),
        _image('n_is_topk', N, 52, passing(topk), dict(n=topk, levels=0))])


# ------------------------------------------------------------------------------------------------------------ D. greedy selection
D_CONF, D_THR, D_N = 0.3, 0.2, 520


def _compose(name, segments, seed, claim, N=D_N):
    """segments: (class id, [(cx, cy)]) in the order the sorted output must have: classes ascending, and inside a class the
    listed order is the score order.  The candidates are shuffled, so the index order is not the sorted one; the rest of the N
    are copies of box 0 that fail the filter."""
    xy = np.concatenate([np.asarray(p, F32).reshape(-1, 2) for _, p in segments])
    cls = np.concatenate([np.full(len(p), c, np.int64) for c, p in segments])
    n = len(xy)
    assert n <= N
    score = np.empty(n, F32)
    at = 0
    for _, p in segments:
        score[at:at + len(p)] = (0.95 - 0.001 * np.arange(len(p))).astype(F32)
        at += len(p)
    rng = _rng(seed)
    perm = rng.permutation(N)[:n]
    b = np.zeros((N, 4), F32)
    b[:, 2:] = 20
    b[:, :2] = xy[0]
    c = np.full(N, cls[0], np.int64)
    s = np.full(N, 0.1, F32)
    b[perm, :2], c[perm], s[perm] = xy, cls, score
    return dict(name=name, b=b, c=c, s=s, claim=dict(claim, n=n, nsel=n, levels=0))


def _chain(boxes, y, x0=0.0):
    """`boxes` boxes, each overlapping only its successor."""
    return [(x0 + 12.0 * i, y) for i in range(boxes)]


def _isolated(k, y):
    return [(40.0 * i, y) for i in range(k)]


def _pairs(k, y):
    """k boxes in overlapping pairs (a 1-link chain each; an odd one out stands alone)."""
    return [(60.0 * (i // 2) + 12.0 * (i & 1), y) for i in range(k)]


def handover_images(links):
    """Chains of the given numbers of links as class 1 of images whose other classes settle in two rounds, nsel = 65, 200, 512."""
    out = []
    for L in links:
        for nsel in (65, 200, 512):
            f0 = 50 if nsel == 65 else 58
            rest = nsel - f0 - (L + 1)
            segs = [(0, _isolated(f0, 0.0)), (1, _chain(L + 1, 100.0)), (2, _pairs(rest, 200.0))]
            out.append(_compose(f'chain_{L}_links_nsel_{nsel}', segs, 1000 + 10 * L + nsel, dict(rounds=max(L + 1, 2))))
    return out


def _d_launches():
    out = []
    interleaved = _compose('three_interleaved_500', [(c, _chain(167 - (c == 2), 100.0 * c)) for c in range(3)], 61, dict(rounds=167))
    out.append(dict(name='D_fallback', conf=D_CONF, thr=D_THR, images=[
        _compose('one_chain_512', [(3, _chain(512, 0.0))], 60, dict(rounds=512)),
        interleaved,
        _compose('chain_from_position_60', [(0, _isolated(60, 0.0)), (1, _chain(301, 100.0)), (2, _pairs(10, 200.0))], 62,
                 dict(rounds=301)),
    ]))
    words = [_compose(f'one_class_{k}', [(2, _chain(k, 0.0))], 70 + k, dict(rounds=k)) for k in (63, 64, 65, 127, 128, 129, 511, 512)]
    words += [_compose(f'two_classes_{p}_{q}', [(1, _chain(p, 0.0)), (4, _chain(q, 100.0))], 80 + p, dict(rounds=max(p, q)))
              for p, q in ((64, 64), (63, 66), (1, 511))]
    out.append(dict(name='D_word_edges', conf=D_CONF, thr=D_THR, images=words))

    def classes(name, seed, ids, bad, low_id=None):
        img = _compose(name, [(0, _pairs(100, 0.0)), (1, _pairs(100, 100.0))], seed, dict(rounds=2, bad=bad))
        del img['claim']['rounds']                                # the ids below regroup the pairs
        sel = plan.passing(img['s'], D_CONF)
        img['c'][sel] = np.asarray(ids, np.int64)[np.arange(len(sel)) % len(ids)]
        if low_id is not None:
            img['c'][img['s'] < D_CONF] = low_id
        return img
    out.append(dict(name='D_class_ids', conf=D_CONF, thr=D_THR, images=[
        classes('ids_0_4095', 90, (0, 4095), False),
        classes('ids_4095_4096', 91, (4095, 4095, 4095, 4096), True),
        classes('id_4096_fails_the_filter', 92, (7, 4095), False, low_id=4096),
        classes('id_minus_1', 93, (0, -1), True),
        classes('ids_0_4095_again', 94, (4095, 0, 0), False),
    ]))
    return out


# ---------------------------------------------------------------------------------------------- E. the pair test on the threshold
F45 = float(F32(0.45))                            # float32(0.45) widened: 0.449999988...
E_PAIRS = {                                       # name: (first box, second box) as corners (x1, y1, x2, y2); exact IoU
    'iou_1/2': ((0, 0, 2, 2), (0, 0, 2, 1)),      # 2 / 4
    'iou_1/4': ((0, 0, 2, 2), (0, 0, 1, 1)),      # 1 / 4
    'iou_1': ((0, 0, 2, 2), (0, 0, 2, 2)),
    'iou_45/100': ((0, 0, 100, 100), (0, 0, 100, 45)),      # 4500 / 10000: the float32 quotient IS float32(0.45)
    'iou_4508/10000': ((0, 0, 100, 100), (0, 0, 92, 49)),
    'iou_4488/10000': ((0, 0, 100, 100), (0, 0, 88, 51)),
    'two_zero_area': ((0, 0, 0, 0), (0, 0, 0, 0)),          # 0 / 0: NaN, both kept
    'zero_area_inside': ((0, 0, 4, 4), (2, 2, 2, 2)),       # 0 / 16
    'negative_width': ((0, 0, 4, 4), (3, 0, 1, 4)),         # area -8: the formula is the oracle's
    'two_negative_width': ((4, 0, 0, 4), (4, 0, 0, 4)),
    'negative_cancels': ((0, 0, 2, 2), (2, 0, 0, 2)),       # areas 4 and -4: 0 / 0
}
E_IOU = {'iou_1/2': 0.5, 'iou_1/4': 0.25, 'iou_1': 1.0, 'iou_45/100': F45, 'iou_4508/10000': 0.4508, 'iou_4488/10000': 0.4488}
E_THRESHOLDS = {'1/2': 0.5, 'below_1/2': float(np.nextafter(0.5, 0.0)), '1/4': 0.25, 'below_1/4': float(np.nextafter(0.25, 0.0)),
                '1': 1.0, 'below_1': float(np.nextafter(1.0, 0.0)), 'f32_0.45': F45, 'below_f32_0.45': float(np.nextafter(F45, 0.0)),
                '0.45': 0.45}


def e_image():
    """One image: pair p is class p, 1000 apart from the others; the first box of a pair has the higher score."""
    names = list(E_PAIRS)
    N = 2 * len(names)
    b, c, s = np.zeros((N, 4), F32), np.zeros(N, np.int64), np.zeros(N, F32)
    for p, name in enumerate(names):
        for q, (x1, y1, x2, y2) in enumerate(E_PAIRS[name]):
            b[2 * p + q] = (1000 * p + (x1 + x2) / 2, (y1 + y2) / 2, x2 - x1, y2 - y1)
            c[2 * p + q] = p
            s[2 * p + q] = 0.9 - 0.1 * q
    return dict(name='pairs', b=b, c=c, s=s, claim=dict(n=N, levels=0))


def e_suppressed(thr):
    """Names of the pairs whose second box a threshold removes, from the exact IoU (in double, the kernel's compare)."""
    return {name for name, v in E_IOU.items() if v > thr}


def _e_launches():
    return [dict(name=f'E_thr_{k}', conf=0.0, thr=v, images=[e_image()]) for k, v in E_THRESHOLDS.items()]


# ------------------------------------------------------------------------------------------------------------------- all launches
def _build():
    out = [dict(name='A_topk', conf=CONF, thr=THR, images=_a_images(30000)),
           dict(name='A4_N200000', conf=CONF, thr=THR, images=_a4_images(200000)),
           dict(name='A_N16384', conf=CONF, thr=THR, images=_all_pass(16384)),
           dict(name='A_N16385', conf=CONF, thr=THR, images=_all_pass(16385))]
    out += _c_launches()
    out.append(dict(name='D_handover', conf=D_CONF, thr=D_THR, images=handover_images((10, 11, 12, 13))))
    out += _d_launches()
    out += _e_launches()
    return out


_LAUNCHES = None


def launches():
    """name -> launch; built once (a second of numpy) and shared: nobody writes to the arrays."""
    global _LAUNCHES
    if _LAUNCHES is None:
        _LAUNCHES = {L['name']: L for L in _build()}
        for L in _LAUNCHES.values():
            for img in L['images']:
                for k in ('b', 'c', 's'):
                    img[k].setflags(write=False)
    return _LAUNCHES


NAMES = ['A_topk', 'A4_N200000', 'A_N16384', 'A_N16385', 'C_negative', 'C_mixed_signs', 'C_subnormal_conf0', 'C_subnormal_conf_tiny',
         'C_inf', 'C_nan_conf_-inf', 'C_nan_conf_0.25', 'C_nan_conf_nan', 'C_signed_zero_boundary', 'C_signed_zero_pairs',
         'D_handover', 'D_fallback', 'D_word_edges', 'D_class_ids'] + [f'E_thr_{k}' for k in E_THRESHOLDS]


def check_claims(L, topk=plan.KMAX):
    """Assert that every image of the launch takes the path its claim names; returns {image name: Plan}."""
    plans = {}
    for img in L['images']:
        claim, what = img['claim'], f"{L['name']}/{img['name']}"
        p = plan.topk_plan(img['s'], L['conf'], topk)
        plans[img['name']] = p
        for field in ('n', 'sweeps', 'levels', 'bins', 'need', 'tail', 'tail_trips'):
            if field in claim:
                assert getattr(p, field) == claim[field], f'{what}: {field} is {getattr(p, field)!r}, the case claims {claim[field]!r}'
        if 'bins4' in claim:
            assert p.bins[:4] == claim['bins4'] and len(p.bins) == 5 and p.bins[4] <= 16, f'{what}: bins {p.bins}'
        if p.levels:
            assert p.list_len == p.bins[-1] <= plan.LIST and 1 <= p.need <= p.list_len, what
        if 'rounds' in claim:
            rounds, nsel = plan.settles(img['b'], img['c'], img['s'], L['conf'], L['thr'], topk)
            assert rounds == claim['rounds'], f"{what}: {rounds} rounds, the case claims {claim['rounds']}"
            if 'nsel' in claim:
                assert nsel == claim['nsel'], f"{what}: nsel {nsel}, the case claims {claim['nsel']}"
    return plans
