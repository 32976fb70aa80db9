"""Inputs of tests/test_gpu_nms_modes.py and of the seed condition in tests/test_nms_modes_host.py.  Numpy only, no GPU.

A launch is  dict(name, conf, thr, min_score, images)  and an image  dict(name, b [N,4], c [N], s [N], angle [N]).  The boxes
are clusters in the style of tests/_pp_cases.py (its grid spacing, its distinct scores, its seeded generator): a cluster is a few
boxes of about 24 px jittered by a few pixels around one grid point, so inside a cluster every pair overlaps, suppression and
decay chains form, a decayed score falls below the next cluster's and the emission order leaves order P.  A cluster's boxes
share a class except every third, which takes the next class: the pairs an agnostic mode must join and a class-aware one must
not.  Scores are distinct (cases._distinct), so order P has no ties except where a test plants one.

SEEDS are fixed.  tests/test_nms_modes_host.py asserts for each that every Gaussian weight the launch computes lies farther
than 2^-45 (relative) from a float32 rounding midpoint; a seed that breaks it is replaced there, on the CPU."""
import numpy as np

import _nms_ref as ref
import _pp_cases as cases

F32 = np.float32
CONF, THR, SIGMA = 0.25, 0.45, 0.5
MODES = [(kind, agn) for kind in ref.KINDS for agn in (False, True) if (kind, agn) != ('hard', False)]


def clustered(name, N, seed, class_ids, passing=None, lo=0.3, hi=1.0):
    """N candidates in clusters of 1..6; `passing` of them (default all) get distinct scores in (lo, hi), the rest fail CONF."""
    rng = cases._rng(seed)
    passing = N if passing is None else passing
    b = np.zeros((N, 4), F32)
    c = np.zeros(N, np.int64)
    i = cell = 0
    while i < N:
        m = min(int(rng.integers(1, 7)), N - i)
        cx, cy = 64.0 * (cell % 16) + 32, 64.0 * (cell // 16) + 32
        base = int(rng.integers(0, len(class_ids)))
        for q in range(m):
            b[i + q] = (cx + rng.integers(-6, 7), cy + rng.integers(-6, 7), 24 + rng.integers(-4, 5), 24 + rng.integers(-4, 5))
            c[i + q] = class_ids[(base + (q % 3 == 2)) % len(class_ids)]
        i += m
        cell += 1
    perm = rng.permutation(N)
    b, c = b[perm], c[perm]
    s = cases._below(N, rng)
    s[np.sort(rng.permutation(N)[:passing])] = cases._distinct(passing, rng, lo, hi)
    angle = (rng.random(N, dtype=F32) * 180 - 90).astype(F32)
    return dict(name=name, b=b, c=c, s=s, angle=angle)


def _build():
    out = []
    for N in (1, 63, 64, 65):
        out.append(dict(name=f'N{N}', conf=CONF, thr=THR, min_score=None, images=[
            clustered('three_classes', N, 100 + N, (0, 1, 2)), clustered('one_class', N, 200 + N, (7,))]))
    out.append(dict(name='N600', conf=CONF, thr=THR, min_score=None, images=[           # 600 pass: the top-k boundary feeds the mode
        clustered('80_classes', 600, 300, tuple(range(80))), clustered('ids_0_5_4095', 600, 301, (0, 5, 4095))]))
    # min_score 0: nothing is cut, so the one-class image runs all 512 dependent picks
    out.append(dict(name='N512', conf=CONF, thr=THR, min_score=0.0, images=[
        clustered('one_class_512', 512, 400, (3,)),                                     # the longest group
        clustered('empty', 512, 401, (0, 1), passing=0),
        clustered('half_pass', 512, 402, (0, 1, 4095), passing=256)]))
    # every group's first pick is below min_score: the soft kinds emit nothing, the others are not concerned
    out.append(dict(name='N65_min_score', conf=CONF, thr=THR, min_score=0.95, images=[
        clustered('below_min_score', 65, 500, (0, 1, 2), hi=0.9)]))
    return out


_LAUNCHES = None
_REF = {}


def launches():
    global _LAUNCHES
    if _LAUNCHES is None:
        _LAUNCHES = {L['name']: L for L in _build()}
        for L in _LAUNCHES.values():
            for img in L['images']:
                for k in ('b', 'c', 's', 'angle'):
                    img[k].setflags(write=False)
    return _LAUNCHES


NAMES = ['N1', 'N63', 'N64', 'N65', 'N600', 'N512', 'N65_min_score']


def expected(name, kind, agnostic):
    """(results of the launch's images, the Stats of the run): computed once, shared, never written to."""
    key = (name, kind, agnostic)
    if key not in _REF:
        L = launches()[name]
        st = ref.Stats()
        _REF[key] = ([ref.run(img['b'], img['c'], img['s'], L['conf'], L['thr'], kind, agnostic, SIGMA, L['min_score'], stats=st)
                      for img in L['images']], st)
    return _REF[key]


def check_branches():
    """The cases meet what they are for: the soft kinds re-order a group relative to P, cut a group on min_score and run 512
    dependent picks; every agnostic mode joins boxes of different classes; merge forms clusters of more than one box.  A case
    list that never takes a branch shows nothing about it."""
    for kind in ('soft-linear', 'soft-gaussian'):
        assert sum(expected(n, kind, a)[1].reordered for n in NAMES for a in (False, True)) > 0, kind
        assert sum(expected(n, kind, True)[1].cross_class for n in NAMES) > 0, kind
        assert expected('N65_min_score', kind, False)[1].cut > 0 and expected('N65_min_score', kind, False)[0][0]['count'] == 0
        assert expected('N512', kind, False)[0][0]['count'] == 512
    for kind in ('hard', 'merge'):
        assert sum(expected(n, kind, True)[1].cross_class for n in NAMES) > 0, kind
    assert sum(expected(n, 'merge', a)[1].merged for n in NAMES for a in (False, True)) > 0
    # N600: more than 512 pass, so the selected list is cut by the top-k before any mode sees it
    L = launches()['N600']
    assert all(int((img['s'] >= F32(L['conf'])).sum()) > 512 for img in L['images'])
