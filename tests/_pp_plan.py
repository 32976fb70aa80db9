"""The launch rules of postprocess_kernel (mydetection_amd/csrc/postprocess.hip), restated on the host.  Numpy only, no GPU.

The kernel picks its path from the data: how many histogram levels the top-k runs, whether keys are re-read from scratch,
whether the greedy NMS settles as a fixed point or hands over to the sequential form.  The functions here say which path an
input takes, so that tests/test_gpu_postprocess_branches.py can assert that each of its cases runs the branch it names, and
tests/test_pp_plan_host.py can hold the restatement itself to oracle.postprocess without a GPU.

    keys(scores, conf)                uint64 keys of the candidates that pass the filter
    topk_plan(scores, conf, topk)     Plan: n, levels, bins, need, tail, ... and the k-th key the search ends on
    order_and_mask(b, c, s, sel, thr) the kernel's sorted order of the selected and their suppression matrix
    rounds_needed(mask)               iterations of the fixed point, the one that changes nothing included
    greedy_from_rounds(mask)          the kept set read from the settled `removed`

Chains.  For a chain of L links (L + 1 boxes, box i suppresses box i + 1 only) rounds_needed is L + 1.  Iteration t builds
removed_t = OR of the rows of the boxes outside removed_(t-1), and a box's row is one bit, its successor.  Box 0 is in no row,
so it is kept from the start; by induction boxes 0..t hold their final state (odd removed, even kept) after iteration t: box t
is set exactly when box t - 1 was kept in removed_(t-1), which is final for t - 1 <= t - 1.  The boxes behind t all still carry
the state of the start, alternating as a block: after an odd iteration every one of them is removed (all boxes were kept
before, so all successors are set), after an even one every one is kept.  So removed_t is final iff no box lies behind t, that
is t >= L: box L is wrong in removed_(L-1) whatever the parity of L.  Iteration L is the first that gives the final set and
iteration L + 1 is the first that changes nothing: L + 1 iterations for L >= 1, and 1 = L + 1 for the single box too.  The
kernel runs MAX_ROUNDS = 12 of them, so a chain of 11 links is the last that settles and one of 12 links the first that
does not (test_pp_plan_host.py finds the two lengths by running rounds_needed, not from this paragraph)."""
from collections import namedtuple

import numpy as np

KMAX = 512            # postprocess.hip: KMAX
NT = 1024             # threads of the workgroup
FU = 16               # score loads in flight per thread in the filter: one sweep covers FU * NT candidates
RK = 16               # keys per thread that stay in registers: RK * NT keys in all
TAIL_STEP = 8 * NT    # keys one trip of the tail loop covers
LIST = 1024           # the histogram rounds stop when the chosen bin holds at most LIST keys
SHIFTS = (52, 40, 28, 16, 4)
MAX_ROUNDS = 12
IDX_BITS = 20
CLASS_LIMIT = 1 << 12


def sortable(scores):
    """sortable() of the kernel on a float32 array: an order-preserving map to uint32, -0.0 taking the key of +0.0."""
    u = np.ascontiguousarray(scores, dtype=np.float32).view(np.uint32).copy()
    u[u == 0x80000000] = 0
    neg = (u & np.uint32(0x80000000)) != 0
    return np.where(neg, ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def passing(scores, conf):
    """Indices of the candidates that pass `score >= conf` in float32 (a NaN never does)."""
    scores = np.asarray(scores, dtype=np.float32)
    with np.errstate(invalid='ignore'):
        return np.nonzero(scores >= np.float32(conf))[0]


def keys(scores, conf):
    """uint64 keys of the passing candidates, in index order: sortable(score) << 32 | (0xFFFFFFFF - index)."""
    scores = np.asarray(scores, dtype=np.float32)
    idx = passing(scores, conf)
    return (sortable(scores[idx]).astype(np.uint64) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - idx.astype(np.uint64))


def key_index(k):
    return (np.uint64(0xFFFFFFFF) - (np.asarray(k, dtype=np.uint64) & np.uint64(0xFFFFFFFF))).astype(np.int64)


Plan = namedtuple('Plan', 'n sweeps levels bins need tail tail_trips list_len bit_steps kth')
Plan.__doc__ = """What the kernel does on one image.
n          candidates that pass the filter
sweeps     trips of the filter loop: ceil(N / (FU * NT))
levels     histogram levels run; 0 when n <= topk (the whole search is skipped)
bins       size of the chosen bin at each level
need       rank of the wanted key inside the last chosen bin, at the exit of the level loop
tail       n > RK * NT: keys are re-read from scratch
tail_trips trips of the tail loop of thread 0 (the thread with the most)
list_len   keys compacted into the LDS list
bit_steps  iterations of the bit-by-bit search (it stops when a candidate cuts off exactly `need`)
kth        the threshold key the search ends on: the selected are the keys >= kth (0 when levels == 0)"""


def topk_plan(scores, conf, topk=KMAX):
    assert 1 <= topk <= KMAX
    N = len(scores)
    k = keys(scores, conf)
    n = len(k)
    sweeps = -(-N // (FU * NT))
    tail = n > RK * NT
    trips = len(range(RK * NT, n, TAIL_STEP))
    if n <= topk:
        return Plan(n, sweeps, 0, (), topk, tail, trips, 0, 0, 0)
    prefix, need, low, bins = 0, topk, 64, []
    match = k
    for shift in SHIFTS:
        if low < 64:
            match = match[(match >> np.uint64(low)) == np.uint64(prefix >> low)]
        hist = np.bincount(((match >> np.uint64(shift)) & np.uint64(4095)).astype(np.int64), minlength=4096)
        above = np.concatenate([np.cumsum(hist[::-1])[::-1][1:], [0]])          # keys in the bins above each bin
        sel = int(np.nonzero((above < need) & (above + hist >= need))[0][0])    # exactly one bin
        prefix |= sel << shift
        need -= int(above[sel])
        low = shift
        bins.append(int(hist[sel]))
        if bins[-1] <= LIST:
            break
    lst = [int(v) for v in match[(match >> np.uint64(low)) == np.uint64(prefix >> low)]]
    steps = 0
    for bit in range(low - 1, -1, -1):
        cand = prefix | (1 << bit)
        cnt = sum(v >= cand for v in lst)
        steps += 1
        if cnt >= need:
            prefix = cand
        if cnt == need:
            break
    return Plan(n, sweeps, len(bins), tuple(bins), need, tail, trips, len(lst), steps, prefix)


def selected(scores, conf, topk=KMAX):
    """Candidate indices the kernel selects (ascending): every passing one, or those whose key is >= the plan's kth."""
    k = keys(scores, conf)
    if len(k) <= topk:
        return np.sort(key_index(k))
    return np.sort(key_index(k[k >= np.uint64(topk_plan(scores, conf, topk).kth)]))


def order_and_mask(bboxes, cats, scores, sel, thr):
    """The selected candidates `sel` in the kernel's sorted order (class ascending, score descending, index ascending; the two
    zeros are one score) and the suppression matrix in that order: mask[i, j] = j > i, same class and (double)IoU > thr, the
    IoU in the oracle's float32 operation order (oracle/nms_ref.c on oracle.postprocess.cxcywh_to_x1y1x2y2)."""
    from oracle.postprocess import cxcywh_to_x1y1x2y2
    sel = np.asarray(sel, dtype=np.int64)
    s = np.asarray(scores, dtype=np.float32)[sel]
    c = np.asarray(cats, dtype=np.int64)[sel]
    order = sel[np.lexsort((sel, -(s + np.float32(0)), c))]                  # x + 0 turns -0 into +0; lexsort: last key first
    b = cxcywh_to_x1y1x2y2(np.asarray(bboxes, dtype=np.float32)[order])
    c = np.asarray(cats, dtype=np.int64)[order]
    x1, y1, x2, y2 = (b[:, i] for i in range(4))
    area = (x2 - x1) * (y2 - y1)
    with np.errstate(invalid='ignore', divide='ignore'):
        w = np.minimum(x2[:, None], x2[None]) - np.maximum(x1[:, None], x1[None])
        h = np.minimum(y2[:, None], y2[None]) - np.maximum(y1[:, None], y1[None])
        w = np.where(w > 0, w, np.float32(0))
        h = np.where(h > 0, h, np.float32(0))
        inter = w * h
        ovr = inter / (area[:, None] + area[None] - inter)
        assert ovr.dtype == np.float32
        mask = ovr.astype(np.float64) > float(thr)
    mask &= c[:, None] == c[None]
    mask &= np.arange(len(order))[:, None] < np.arange(len(order))[None]
    return order, mask


def rounds_needed(mask):
    """Iterations of  removed <- OR of the rows of the boxes not removed  from removed = 0 until one changes nothing, that
    one included.  mask: boolean, upper triangular.  The kernel settles iff the count is at most MAX_ROUNDS."""
    mask = np.asarray(mask, dtype=bool)
    removed = np.zeros(mask.shape[0], dtype=bool)
    count = 0
    while True:
        new = mask[~removed].any(axis=0)
        count += 1
        if np.array_equal(new, removed):
            return count
        removed = new


def greedy_from_rounds(mask):
    """Positions kept by the fixed point: the complement of the settled `removed`."""
    mask = np.asarray(mask, dtype=bool)
    removed = np.zeros(mask.shape[0], dtype=bool)
    while True:
        new = mask[~removed].any(axis=0)
        if np.array_equal(new, removed):
            return np.nonzero(~removed)[0]
        removed = new


def settles(bboxes, cats, scores, conf, thr, topk=KMAX):
    """(rounds, nsel) of one image: rounds_needed of its whole suppression matrix (classes are independent blocks, so this is
    the largest count of any class) and the number of selected candidates."""
    sel = selected(scores, conf, topk)
    if len(sel) == 0:
        return 1, 0
    _, mask = order_and_mask(bboxes, cats, scores, sel, thr)
    return rounds_needed(mask), len(sel)
