"""The whole track scorer as plain Python / numpy (test code; the package never imports it).

Written from the rule text of include/mydet.h ("Scoring tracks against ground truth"), not from the package's code: it takes the
JSON lists directly and does its own packing with dictionaries, so it checks the packer as well.  `evaluate` returns every array
in the layout the rules give the device arrays, so a test compares them with ==.  The axis-aligned IoU is tests/_eval_ref.iou_axis
(float64, the documented order); the rotated one is tests/_rotbox_ref.iou_matrix on the float32-rounded rows.
"""
import itertools

import numpy as np

import _eval_ref
import _rotbox_ref

ONE, BIG, INF = 65536, 1 << 27, 1 << 60
ID_KEYS = ('track_id', 'person_id')


def assign(cost):
    """The shortest-augmenting-path Hungarian method, u / v / p / way / minv form, on an integer matrix [n][m]: rows inserted in
    ascending order, the next column the unused one of least minv (lowest index on a tie), transposed first when n > m.
    Returns (col_of_row list with -1 for an unassigned row, total)."""
    a = np.asarray(cost, dtype=np.int64)
    n, m = a.shape
    if n == 0 or m == 0:
        return [-1] * n, 0
    if n > m:
        row_of_col, total = assign(a.T)                               # its rows are our columns
        col_of_row = [-1] * n
        for c, r in enumerate(row_of_col):
            if r >= 0:
                col_of_row[r] = c
        return col_of_row, total
    u, v = np.zeros(n, np.int64), np.zeros(m, np.int64)
    p = np.full(m, -1, np.int64)
    way = np.full(m, -1, np.int64)
    for i in range(n):
        minv = np.full(m, INF, np.int64)
        used = np.zeros(m, bool)
        j0 = -1
        while True:
            if j0 >= 0:
                used[j0] = True
            i0 = i if j0 < 0 else p[j0]
            cur = a[i0] - u[i0] - v
            better = ~used & (cur < minv)
            minv[better] = cur[better]
            way[better] = j0
            masked = np.where(used, np.int64(INF) * 2, minv)
            j1 = int(np.argmin(masked))                               # the first minimum: the lowest column index
            delta = masked[j1]
            u[p[used]] += delta
            u[i] += delta
            v[used] -= delta
            minv[~used] -= delta
            j0 = j1
            if p[j0] < 0:
                break
        while j0 >= 0:
            j1 = int(way[j0])
            p[j0] = i if j1 < 0 else p[j1]
            j0 = j1
    col_of_row = [-1] * n
    for j in range(m):
        if p[j] >= 0:
            col_of_row[int(p[j])] = j
    return col_of_row, int(sum(a[r, c] for r, c in enumerate(col_of_row)))


def brute_force(cost):
    """The least total over all one-to-one assignments of the smaller side."""
    a = np.asarray(cost, dtype=np.int64)
    if a.shape[0] > a.shape[1]:
        a = a.T
    n, m = a.shape
    return min(int(sum(a[r, c] for r, c in enumerate(perm))) for perm in itertools.permutations(range(m), n))


def pair_cost(iou, thr):
    """(eligible, cost) of one pair."""
    ok = bool(iou >= thr)                                            # NaN: False
    return ok, (ONE - int(np.floor(np.float64(iou) * 65536.0))) if ok else BIG


def sequences_of(gt, sequences=None):
    images = gt['images']
    if sequences is not None:
        return list(sequences), [list(v) for v in sequences.values()]
    if images and all('video_id' in im and 'frame_id' in im for im in images):
        names = sorted(set(im['video_id'] for im in images))
        return names, [[im['id'] for im in sorted((im for im in images if im['video_id'] == n), key=lambda im: im['frame_id'])] for n in names]
    return ['all'], [[im['id'] for im in images]]


def evaluate(dts, gt, kind, thrs, sequences=None, id_key=None, use_cats=True, ious=None):
    """Everything the device computes: ious, counts [U,T,5], siou [U,T], present [Gids], matched [T,Gids], gt_match [T,G],
    overlap [T, n_ov] (the flat matrices, unit after unit), idtp [U,T], plus the tables.  `ious`: a flat buffer to use instead of the
    computed one (the same layout), for tests that set pair values directly."""
    rotated, ious_given = kind == 'cepdof', ious
    thrs = [float(t) for t in thrs]
    T = len(thrs)
    names, frames = sequences_of(gt, sequences)
    S = len(names)
    cat_ids = sorted(set(c['id'] for c in gt['categories'])) if use_cats else [None]
    K = len(cat_ids)
    key = id_key if id_key is not None else next(k for k in ID_KEYS if all(k in a for a in gt['annotations']))
    where = {}                                                        # image id -> (sequence, frame in the sequence)
    for s, ids in enumerate(frames):
        for f, i in enumerate(ids):
            where[i] = (s, f)

    def cat_index(c):
        return (cat_ids.index(c) if c in cat_ids else -1) if use_cats else 0

    # units[k][s][f] = (hypotheses, ground truths) of the frame, input order
    units = [[[([], []) for _ in ids] for ids in frames] for _ in range(K)]
    for n, a in enumerate(gt['annotations']):
        k = cat_index(a.get('category_id', 1))
        if a['image_id'] in where and k >= 0:
            s, f = where[a['image_id']]
            units[k][s][f][1].append({'row': n, 'box': a['bbox'], 'id': a[key]})
    for n, d in enumerate(dts):
        k = cat_index(d.get('category_id', 1) if rotated else d['category_id'])
        if d['image_id'] in where and k >= 0:
            s, f = where[d['image_id']]
            units[k][s][f][0].append({'row': n, 'box': d['bbox'], 'id': d['track_id']})

    # dense numbering in group order g = k*I + frame, units u = k*S + s
    out = {'S': S, 'K': K, 'U': S * K, 'seq_names': names}
    e_d = e_g = 0
    ious, dt_rows, gt_rows = [], [], []
    gt_id_start, dt_id_start = [0], [0]
    for k in range(K):
        for s in range(S):
            g_ids, h_ids = {}, {}
            for hyps, gts in units[k][s]:
                for d in hyps:
                    d['e'], d['dense'] = e_d, h_ids.setdefault(d['id'], len(h_ids))
                    e_d += 1
                    dt_rows.append(d['row'])
                for j in gts:
                    j['e'], j['dense'] = e_g, g_ids.setdefault(j['id'], len(g_ids))
                    e_g += 1
                    gt_rows.append(j['row'])
                assert len(set(d['dense'] for d in hyps)) == len(hyps) and len(set(j['dense'] for j in gts)) == len(gts)
            gt_id_start.append(gt_id_start[-1] + len(g_ids))
            dt_id_start.append(dt_id_start[-1] + len(h_ids))
    # the dense numbering above runs unit-major (k, s, frame), which is group order because sequences are laid end to end
    D, G = e_d, e_g
    for k in range(K):
        for s in range(S):
            for hyps, gts in units[k][s]:
                if hyps and gts:
                    if rotated:
                        a = np.array([d['box'][:5] for d in hyps], np.float32).astype(np.float64)
                        b = np.array([j['box'][:5] for j in gts], np.float32).astype(np.float64)
                        block = _rotbox_ref.iou_matrix(a, b)
                    else:
                        block = np.array([[_eval_ref.iou_axis(d['box'], j['box'], False) for j in gts] for d in hyps], np.float64)
                    block = np.asarray(block, np.float64).reshape(len(hyps), len(gts))
                else:
                    block = np.zeros((len(hyps), len(gts)))
                ious.append(block)
    if ious_given is not None:
        flat, at = np.asarray(ious_given, np.float64), 0
        for n, b in enumerate(ious):
            ious[n] = flat[at:at + b.size].reshape(b.shape)
            at += b.size
        assert at == flat.size
    out['ious'] = np.concatenate([b.ravel() for b in ious]) if ious else np.zeros(0)
    out.update(D=D, G=G, dt_rows=np.array(dt_rows, np.int64), gt_rows=np.array(gt_rows, np.int64),
               gt_id_start=np.array(gt_id_start, np.int32), dt_id_start=np.array(dt_id_start, np.int32))

    Gids = gt_id_start[-1]
    counts = np.zeros((S * K, T, 5), np.int64)
    siou = np.zeros((S * K, T), np.float64)
    present = np.zeros(Gids, np.int32)
    matched = np.zeros((T, Gids), np.int32)
    gt_match = np.full((T, G), -1, np.int32)
    idtp = np.zeros((S * K, T), np.int64)
    overlap = [[] for _ in range(T)]
    block_of = iter(ious)
    blocks = [[[next(block_of) for _ in units[k][s]] for s in range(S)] for k in range(K)]
    for k in range(K):
        for s in range(S):
            u = k * S + s
            n_g, n_h = gt_id_start[u + 1] - gt_id_start[u], dt_id_start[u + 1] - dt_id_start[u]
            for t, thr in enumerate(thrs):
                last, ever, prev = [-1] * n_g, [False] * n_g, [False] * n_g
                n = np.zeros((n_g, n_h), np.int64)
                tp = fp = fn = idsw = frag = 0
                total = np.float64(0.0)
                for (hyps, gts), iou in zip(units[k][s], blocks[k][s]):
                    match = [-1] * len(gts)
                    free = [True] * len(hyps)
                    col_of = {d['dense']: c for c, d in enumerate(hyps)}
                    for r, j in enumerate(gts):
                        for c, d in enumerate(hyps):
                            if iou[c, r] >= thr:
                                n[j['dense'], d['dense']] += 1
                    for r, j in enumerate(gts):                        # 1. keep
                        c = col_of.get(last[j['dense']], -1) if last[j['dense']] >= 0 else -1
                        if c >= 0 and iou[c, r] >= thr and free[c]:
                            match[r], free[c] = c, False
                    rows = [r for r in range(len(gts)) if match[r] < 0]
                    cols = [c for c in range(len(hyps)) if free[c]]
                    if rows and cols:                                 # 2. assign
                        cost = [[pair_cost(iou[c, r], thr)[1] for c in cols] for r in rows]
                        col_of_row, _ = assign(cost)
                        for i, jj in enumerate(col_of_row):
                            if jj >= 0 and iou[cols[jj], rows[i]] >= thr:
                                match[rows[i]] = cols[jj]
                    for r, j in enumerate(gts):                        # 3. and 4.
                        o = j['dense']
                        if match[r] >= 0:
                            h = hyps[match[r]]['dense']
                            tp += 1
                            total = total + iou[match[r], r]
                            idsw += last[o] >= 0 and last[o] != h
                            frag += ever[o] and not prev[o]
                            last[o], ever[o], prev[o] = h, True, True
                            matched[t, gt_id_start[u] + o] += 1
                            gt_match[t, j['e']] = hyps[match[r]]['e']
                        else:
                            prev[o] = False
                            fn += 1
                        if t == 0:
                            present[gt_id_start[u] + o] += 1
                    fp += len(hyps) - sum(m >= 0 for m in match)
                counts[u, t] = (tp, fp, fn, idsw, frag)
                siou[u, t] = total
                overlap[t].append(n.ravel())
                if n_g and n_h:
                    F = len(units[k][s])
                    col_of_row, _ = assign(F - n)
                    idtp[u, t] = sum(int(n[r, c]) for r, c in enumerate(col_of_row) if c >= 0)
    out.update(counts=counts, siou=siou, present=present, matched=matched, gt_match=gt_match, idtp=idtp,
               overlap=np.stack([np.concatenate(o) if o else np.zeros(0, np.int64) for o in overlap]).astype(np.int32))
    return out


def metrics(tp, fp, fn, idsw, frag, siou, idtp, present, matched):
    """One row of the summary from exact integers: every ratio one float64 division."""
    def ratio(a, b):
        return float(np.float64(a) / np.float64(b)) if b else float('nan')
    n_gt, n_hyp = tp + fn, tp + fp
    mt = sum(5 * m >= 4 * p for m, p in zip(matched, present))
    ml = sum(5 * m < p for m, p in zip(matched, present))
    return {'tp': tp, 'fp': fp, 'fn': fn, 'idsw': idsw, 'frag': frag, 'n_gt': n_gt, 'n_hyp': n_hyp, 'idtp': idtp,
            'idfp': n_hyp - idtp, 'idfn': n_gt - idtp, 'mota': 1.0 - ratio(fn + fp + idsw, n_gt), 'motp': ratio(siou, tp),
            'precision': ratio(tp, n_hyp), 'recall': ratio(tp, n_gt), 'idf1': ratio(2 * idtp, n_gt + n_hyp),
            'idp': ratio(idtp, n_hyp), 'idr': ratio(idtp, n_gt), 'n_ids': len(present), 'mt': mt, 'pt': len(present) - mt - ml, 'ml': ml}
