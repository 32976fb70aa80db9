"""GPU: every branch of postprocess_kernel (mydetection_amd/csrc/postprocess.hip) against oracle.postprocess.post_process.

The kernel picks its path from the data: how many 4096-bin histogram levels the top-k runs, whether keys are re-read from
scratch, whether the greedy NMS settles as a fixed point or takes the sequential form, which 64-box words of the suppression
mask a row walks.  Each case below is an input that the rules send down one path on purpose.  The inputs and the path each one
claims are in tests/_pp_cases.py, the rules are restated in tests/_pp_plan.py, and every test asserts the claims of its launch
(cases.check_claims) before it launches; tests/test_pp_plan_host.py asserts the same claims without a GPU.

  case (launch / image)                 runs                                                             postprocess.hip
  ------------------------------------  ---------------------------------------------------------------  ---------------
  A_topk / A0_512_pass                  n == topk: the search is skipped, kth = 0                        137
  A_topk / A1_513_tied, _two_scores     one level; need = 512 of a one-bin list of 513 / the boundary    160-204, 222-233
                                        between two scores (need == in_bin == 512)
  A_topk / A2_20000_distinct            two levels; keys 16 384.. re-read by the tail loop               147-156, 203
  A_topk / A3_ulps                      three levels: 0.5 + k ulps, only level 2's low score bits tell   160-204
                                        them apart (bins 2048, 2048, 8)
  A4_N200000 / A4_every_100th           four levels: level 3 works on index bits 27..16 (bins 2000 x3,   160-204
                                        656); 13 sweeps of the filter
  A_topk / A5_3000_contiguous           five levels (3000 x4, 16); the list holds <= 16 keys, 4 bits     160-204, 222-233
  A4_N200000 / five_levels_across_65536 five levels with a split at level 3 (1536 of 3000)               160-204
  A_topk / A6_all_equal                 five levels on 30 000 keys, need == in_bin == 16, 2 tail trips   147-156, 160-204
  A_topk / LIST_1024, LIST_1025         in_bin <= LIST decided both ways: one level / five levels        203, 209-219
  A_topk / need_1, need_whole_bin       need == 1 and need == in_bin of a tied bin                       185-201, 222-233
  A_topk / n_16384, n_16385, n_24577    last key in registers, first key outside, second tail trip       144, 147-156
  A_topk / empty, few_100               n == 0 and n <= topk beside the others: scratch offset b * N     91, 137
  A_N16384, A_N16385                    one filter sweep of FU * NT, and one candidate more (the         102-123
                                        clamped load of the last sweep)
  B_topk_{1,2,63,64,65,511}             run-time topk: need = topk, zero fill of rows count..topk,       137, 158, 477-490
                                        nothing written behind row topk (guard words)
  B rejected                            topk 0 / 513: MYDET_E_BADARG; N = 2^20: MYDET_E_UNSUPP           512-513
  C_negative                            sortable()'s branch for negative floats, conf = -inf, -inf       64-70, 112
  C_mixed_signs                         the boundary among negative scores, conf = -0.25                 64-70
  C_subnormal_conf0 / _conf_tiny        subnormal scores and a subnormal conf: nothing is flushed        112
  C_inf                                 +inf scores, 600 of them across the boundary                     64-70
  C_nan_conf_{-inf,0.25,nan}            NaN scores of either sign never pass `>=`                        112
  C_signed_zero_boundary / _pairs       -0.0 and +0.0 are one score in the top-k key and in the class    64-70, 254
                                        sort key; out_score keeps the candidate's bits                   472
  D_handover / chain_{10..13}_links     fixed point of 11, 12 rounds settles; 13, 14 hand over to the    350, 363-392, 397
                                        sequential form; nsel 65, 200, 512 beside settled classes
  D_fallback / one_chain_512            sequential form, all 8 chunks, every carry into a later word     397-435
  D_fallback / three_interleaved_500    sequential form, nsel % 64 != 0 (nb = 52), segments 167,167,166  412, 302-310
  D_fallback / chain_from_position_60   a chain that starts at bit 60 of word 0                          410-418
  D_word_edges / one_class_{63..512}    `w * 64 < e` at e = 63, 64, 65, 127, 128, 129, 511, 512          319
  D_word_edges / two_classes_*          segment ends on / before / after a word edge: s_segend           302-310, 319
  D_class_ids                           4095 sorts last; 4096 or -1 among the selected: count -1, zero   253, 451, 491
                                        rows, neighbours untouched; 4096 below conf: not selected
  E_thr_*                               (double)ovr > thr on exact IoUs 1/2, 1/4, 1, float32(0.45);      329-336
                                        0 / 0 = NaN keeps both; negative widths follow the formula
  BW = 5 (test_five_wide_rows_*)        the <5, false> instance: columns 0-3 decide, the angle travels   288-291, 460-469

What every launch checks, image by image: the count, the kept candidate indices and their order equal the oracle's; boxes,
scores and classes are bit-equal copies of the inputs; rows from the count to topk are zero words.  ops.postprocess (records) and
ops.postprocess_dense give the same words, and a second run gives the same words as the first (the order of the filter's scratch
strip varies between runs).  Nothing here has a tolerance: the kernel's outputs are indices and copies."""
import numpy as np
import pytest
import torch

import _pp_cases as cases
from _arena import SENTINEL_BITS

pytestmark = pytest.mark.gpu

FIELDS = ('bbox', 'score', 'class_idx', 'index')


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    from mydetection_amd import _lib
    _lib.lib()                                   # fail loudly if the HIP library is missing
    return torch.device('cuda:0')


_ORACLE = {}


def _oracle(L, i, topk=512):
    """post_process of image i of a launch: computed once, shared by the tests that run the launch, never written to."""
    from oracle import postprocess as pp
    key = (L['name'], i, topk)
    if key not in _ORACLE:
        img = L['images'][i]
        _ORACLE[key] = pp.post_process(img['b'], img['c'], img['s'], L['conf'], L['thr'], topk)
    return _ORACLE[key]


def _angles(L):
    """An angle column for the five-wide instance: any values, they decide nothing."""
    rng = np.random.Generator(np.random.PCG64(77))
    return [(rng.random(len(img['s']), dtype=np.float32) * 180 - 90).astype(np.float32) for img in L['images']]


def _inputs(L, dev, width=4):
    b = np.stack([img['b'] for img in L['images']])
    if width == 5:
        b = np.concatenate([b, np.stack(_angles(L))[..., None]], axis=2)
    c = np.stack([img['c'] for img in L['images']])
    s = np.stack([img['s'] for img in L['images']])
    return torch.from_numpy(b).to(dev), torch.from_numpy(c).to(dev), torch.from_numpy(s).to(dev)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _check_image(L, i, out, topk, what, angles=None):
    """out: host arrays count (int), bbox [topk, 4 or 5], score, class_idx, index of image i."""
    img = L['images'][i]
    what = f"{L['name']}/{img['name']} {what}"
    for f in FIELDS:
        assert len(out[f]) == topk
    if img['claim'].get('bad'):
        assert out['count'] == -1, f"{what}: count {out['count']} for an image with a class id outside [0, 4096)"
        k = 0
    else:
        ob, oc, os_, src = _oracle(L, i, topk)
        k = out['count']
        assert k == len(src), f'{what}: {k} detections, the oracle has {len(src)}'
        np.testing.assert_array_equal(out['index'][:k].astype(np.int64), src, err_msg=what)
        np.testing.assert_array_equal(_bits(out['score'][:k]), _bits(os_), err_msg=f'{what}: scores are not the input bits')
        np.testing.assert_array_equal(out['class_idx'][:k], oc, err_msg=what)
        np.testing.assert_array_equal(_bits(out['bbox'][:k, :4]), _bits(ob), err_msg=f'{what}: boxes are not the input bits')
        if angles is not None:
            np.testing.assert_array_equal(_bits(out['bbox'][:k, 4]), _bits(angles[i][src]), err_msg=f'{what}: angles')
    for f in FIELDS:
        assert not _bits(out[f][k:]).any(), f'{what}: {f} rows {k}..{topk - 1} are not zero'
    return k


def _host(rec, i, width=4):
    """Image i of a record dict or of a dense dict as host arrays."""
    bbox = rec['bbox'][i].cpu().numpy()
    if 'angle' in rec:
        bbox = np.concatenate([bbox, rec['angle'][i].cpu().numpy()[:, None]], axis=1)
    return dict(count=int(rec['count'][i]), bbox=bbox, score=rec['score'][i].cpu().numpy(),
                class_idx=rec['class_idx'][i].cpu().numpy(), index=rec['index'][i].cpu().numpy())


def _run(dev, L, width=4):
    """Claims, records twice, dense once; every image against the oracle.  Returns the index rows [B, 512] and counts."""
    from mydetection_amd import ops
    cases.check_claims(L)
    tb, tc, ts = _inputs(L, dev, width)
    angles = _angles(L) if width == 5 else None
    rec = ops.postprocess(tb, tc, ts, L['conf'], L['thr'])
    first = rec['records'].clone()
    again = ops.postprocess(tb, tc, ts, L['conf'], L['thr'])['records']
    dense = ops.postprocess_dense(tb, tc, ts, L['conf'], L['thr'], topk=512)
    torch.cuda.synchronize()
    assert torch.equal(first, again), f"{L['name']}: a second run gives other words"
    for i in range(len(L['images'])):
        r, d = _host(rec, i), _host(dense, i)
        _check_image(L, i, r, 512, 'records', angles)
        assert r['count'] == d['count'], f"{L['name']} image {i}: dense count {d['count']}, records {r['count']}"
        for f in FIELDS:
            np.testing.assert_array_equal(_bits(r[f]), _bits(d[f]), err_msg=f"{L['name']} image {i}: dense {f} differs from the record")
    return rec['index'].cpu().numpy(), rec['count'].cpu().numpy()


# --------------------------------------------------------------------------------------------- A, C, D: one test per launch
@pytest.mark.parametrize('name', [n for n in cases.NAMES if n[0] in 'ACD'])
def test_branch(dev, name):
    L = cases.launches()[name]
    index, count = _run(dev, L)
    by_name = {img['name']: i for i, img in enumerate(L['images'])}
    if name == 'A_topk':
        assert count[by_name['empty']] == 0
    if name == 'C_signed_zero_boundary':
        # what the oracle comparison above already holds, said directly: indices 0..511 are selected, 256 of them -0.0,
        # and of each cell's two candidates (IoU 0.6) the lower index stays
        for i in range(2):
            np.testing.assert_array_equal(np.sort(index[i, :count[i]]), np.arange(0, 512, 2))
    if name == 'C_signed_zero_pairs':
        np.testing.assert_array_equal(np.sort(index[0, :count[0]]), np.arange(0, 400, 2))
    if name == 'D_class_ids':
        assert list(count) == [count[0], -1, count[2], -1, count[4]] and min(count[0], count[2], count[4]) > 0
        i = by_name['ids_0_4095']
        cls = np.asarray(L['images'][i]['c'])[index[i, :count[i]]]
        assert cls[0] == 0 and cls[-1] == 4095 and (np.diff(cls) >= 0).all()
    if name == 'D_fallback':
        assert count[by_name['one_chain_512']] == 256           # every other box of the 511-link chain


# ------------------------------------------------------------------------------------------------------ B. topk through the dense ABI
GUARD = 64        # int32 words on either side of every output array (a multiple of 4: the body stays 16-byte aligned)


def _guarded(words, dev):
    """[guard | words | guard] of int32, every word the sentinel; returns (flat, body)."""
    flat = torch.full((2 * GUARD + words,), SENTINEL_BITS, dtype=torch.int32, device=dev)
    return flat, flat[GUARD:GUARD + words]


@pytest.mark.parametrize('topk', cases.B_TOPKS)
def test_topk_below_512_writes_its_rows_only(dev, topk):
    """mydet_postprocess_f32 with its own output buffers: rows below topk are the oracle's at that topk and all defined, the
    words behind row topk of the last image and in front of the first are untouched (a write behind row topk of an earlier
    image lands in the next image's rows, which are compared)."""
    from mydetection_amd import _lib
    from mydetection_amd.ops import _ptr, _stream
    L = cases.b_launch(topk)
    cases.check_claims(L, topk)
    tb, tc, ts = _inputs(L, dev)
    B, N = ts.shape
    bufs = {'count': _guarded(B, dev), 'bbox': _guarded(B * topk * 4, dev), 'class_idx': _guarded(B * topk * 2, dev),
            'score': _guarded(B * topk, dev), 'index': _guarded(B * topk, dev)}
    scratch = torch.empty((B, N), dtype=torch.int64, device=dev)
    code = _lib.lib().mydet_postprocess_f32(_ptr(tb), _ptr(tc), _ptr(ts), B, N, float(L['conf']), float(L['thr']), topk,
                                            *(_ptr(bufs[k][1]) for k in ('count', 'bbox', 'class_idx', 'score', 'index')),
                                            _ptr(scratch), _stream())
    assert code == 0
    torch.cuda.synchronize()
    for name, (flat, body) in bufs.items():
        flat = flat.cpu()
        assert bool((flat[:GUARD] == SENTINEL_BITS).all()), f'topk {topk}: words in front of {name} were written'
        assert bool((flat[GUARD + body.numel():] == SENTINEL_BITS).all()), f'topk {topk}: words behind row topk of {name} were written'
        assert not bool((flat[GUARD:GUARD + body.numel()] == SENTINEL_BITS).any()), f'topk {topk}: words of {name} below row topk were never written'
    host = {k: v[1].cpu() for k, v in bufs.items()}
    for i in range(B):
        out = dict(count=int(host['count'][i]),
                   bbox=host['bbox'].view(torch.float32).view(B, topk, 4)[i].numpy(),
                   score=host['score'].view(torch.float32).view(B, topk)[i].numpy(),
                   class_idx=host['class_idx'].view(torch.int64).view(B, topk)[i].numpy(),
                   index=host['index'].view(B, topk)[i].numpy())
        k = _check_image(L, i, out, topk, f'topk {topk}')
        assert k <= min(topk, L['images'][i]['claim']['n'])
    # ops.postprocess_dense is the same call
    from mydetection_amd import ops
    dense = ops.postprocess_dense(tb, tc, ts, L['conf'], L['thr'], topk=topk)
    for i in range(B):
        _check_image(L, i, _host(dense, i), topk, f'postprocess_dense topk {topk}')


def test_rejected_arguments(dev):
    """topk outside 1..512 is MYDET_E_BADARG and N >= 2^20 MYDET_E_UNSUPP, both before any launch: the outputs stay as they were."""
    from mydetection_amd import _lib
    from mydetection_amd.ops import _ptr, _stream
    B, N = 1, 16
    tb = torch.ones((B, N, 4), device=dev)
    tc = torch.zeros((B, N), dtype=torch.int64, device=dev)
    ts = torch.ones((B, N), device=dev)
    outs = [torch.full((B * 512 * w,), SENTINEL_BITS, dtype=torch.int32, device=dev) for w in (1, 4, 2, 1, 1)]
    scratch = torch.empty((B, N), dtype=torch.int64, device=dev)

    def call(n, topk):
        return _lib.lib().mydet_postprocess_f32(_ptr(tb), _ptr(tc), _ptr(ts), B, n, 0.5, 0.5, topk, *(_ptr(o) for o in outs),
                                                _ptr(scratch), _stream())
    assert call(N, 0) == -1 and call(N, 513) == -1 and call(N, -5) == -1            # MYDET_E_BADARG
    assert call(1 << 20, 512) == -2 and call((1 << 20) + 1, 1) == -2                # MYDET_E_UNSUPP
    torch.cuda.synchronize()
    assert all(bool((o == SENTINEL_BITS).all()) for o in outs)
    assert call(N, 512) == 0                                                        # the same buffers are a valid call
    torch.cuda.synchronize()
    assert int(outs[0][0]) == 1                                                     # 16 copies of one box: one survives


# ------------------------------------------------------------------------------------------------ E. the pair test on the threshold
@pytest.mark.parametrize('thr_name', list(cases.E_THRESHOLDS))
def test_pair_test_on_the_threshold(dev, thr_name):
    L = cases.launches()[f'E_thr_{thr_name}']
    index, count = _run(dev, L)
    kept = set(index[0, :count[0]].tolist())
    names = list(cases.E_PAIRS)
    want = cases.e_suppressed(L['thr'])
    for p, name in enumerate(names):
        assert 2 * p in kept, f'{name}: the first box of a pair always stays'
        if name in cases.E_IOU:
            assert (2 * p + 1 not in kept) == (name in want), f"{name} at thr {L['thr']!r}: IoU {cases.E_IOU[name]!r} > thr is {name in want}"
    for name in ('two_zero_area', 'zero_area_inside'):
        assert 2 * names.index(name) + 1 in kept, f'{name}: kept at every threshold'
    if thr_name in ('1/2', '1/4', '1'):                     # IoU == thr: kept
        assert 2 * names.index(f'iou_{thr_name}') + 1 in kept
    if thr_name.startswith('below_1'):                      # thr one double below the IoU: suppressed
        assert 2 * names.index('iou_' + thr_name[6:]) + 1 not in kept


# -------------------------------------------------------------------------------------------------------------- five-wide rows
@pytest.mark.parametrize('name', ['A_topk', 'C_negative', 'C_signed_zero_boundary', 'D_fallback', 'D_class_ids', 'E_thr_1/2'])
def test_five_wide_rows_decide_like_four_wide(dev, name):
    """The BW = 5 plain instance on the same candidates plus an angle column: the oracle's indices again (what BW = 4 gives in
    the tests above), and each angle beside its box."""
    _run(dev, cases.launches()[name], width=5)


def test_five_wide_rows_at_topk_65(dev):
    from mydetection_amd import ops
    L = cases.b_launch(65)
    tb, tc, ts = _inputs(L, dev, 5)
    dense = ops.postprocess_dense(tb, tc, ts, L['conf'], L['thr'], topk=65)
    for i in range(len(L['images'])):
        out = _host(dense, i)
        _check_image(L, i, out, 65, 'five-wide topk 65', _angles(L))
