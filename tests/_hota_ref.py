"""The HOTA scorer as plain Python / numpy (test code; the package never imports it).

Written from the rule text of include/mydet.h ("HOTA"), not from the package's code: it takes the JSON lists directly and does its
own packing with dictionaries.  `evaluate` returns every array in the layout the rules give the device arrays, so a test compares
the integer ones with ==.  The assignment is tests/_mot_ref.assign as it stands; the axis-aligned IoU is tests/_eval_ref.iou_axis
and the rotated one tests/_rotbox_ref.iou_matrix on the float32-rounded rows.  The two float sums are math.fsum: the correctly
rounded sum of their terms.
"""
import math

import numpy as np

import _eval_ref
import _mot_ref
import _rotbox_ref

P_ONE, Q_ONE = 1 << 30, 1 << 20
DEFAULT_ALPHAS = [n / 20.0 for n in range(1, 20)]


def _value(v):
    v = float(v)
    return 0.0 if v != v else v                                       # a NaN pair value counts as 0


def pair_scores(block, P, gcount, hcount):
    """Rule 2 for one group: block [columns][rows] of IoUs; P, gcount, hcount per (row, column), row and column."""
    q = np.zeros(block.shape, np.int64)
    for c in range(block.shape[0]):
        for r in range(block.shape[1]):
            p = int(P[r][c])
            if p > 0:
                A = float(p) / float((int(gcount[r]) + int(hcount[c])) * P_ONE - p)
                q[c, r] = math.floor(A * _value(block[c, r]) * 1048576.0)
    return q


def evaluate(dts, gt, kind, alphas=None, sequences=None, id_key=None, use_cats=True, ious=None, unlisted=()):
    """Everything the device computes: ious, pot [n_ov], gt_count [Gids], dt_count [Hids], score_q [n_pairs], hota_match [G],
    counts [U,T,3], matches [T,n_ov], loc_sum [U,T], ass_sum [U,T,3], plus n_loc [U,T] and n_ass [U,T], the numbers of terms of
    the two float sums.  `ious`: a flat buffer to use instead of the computed one (the same layout).  `unlisted`: groups
    g = k*I + frame that the caller took out of the list of groups: they have no block in the buffer and take no part."""
    rotated = kind == 'cepdof'
    alphas = [float(a) for a in (DEFAULT_ALPHAS if alphas is None else alphas)]
    T = len(alphas)
    names, frames = _mot_ref.sequences_of(gt, sequences)
    S, I = len(names), sum(len(ids) for ids in frames)
    cat_ids = sorted(set(c['id'] for c in gt['categories'])) if use_cats else [None]
    K = len(cat_ids)
    key = id_key if id_key is not None else next(k for k in _mot_ref.ID_KEYS if all(k in a for a in gt['annotations']))
    where, first = {}, []
    for s, ids in enumerate(frames):
        first.append(len(where))
        for f, i in enumerate(ids):
            where[i] = (s, f)

    def cat_index(c):
        return (cat_ids.index(c) if c in cat_ids else -1) if use_cats else 0

    units = [[[([], []) for _ in ids] for ids in frames] for _ in range(K)]          # [k][s][f] = (hypotheses, ground truths)
    for a in gt['annotations']:
        k = cat_index(a.get('category_id', 1))
        if a['image_id'] in where and k >= 0:
            s, f = where[a['image_id']]
            units[k][s][f][1].append({'box': a['bbox'], 'id': a[key]})
    for d in dts:
        k = cat_index(d.get('category_id', 1) if rotated else d['category_id'])
        if d['image_id'] in where and k >= 0:
            s, f = where[d['image_id']]
            units[k][s][f][0].append({'box': d['bbox'], 'id': d['track_id']})

    # packed row numbers, dense identities per unit, and the IoU blocks, all in group order g = k*I + frame
    e_d = e_g = 0
    gid_start, hid_start, ov_start, blocks = [0], [0], [0], []
    for k in range(K):
        for s in range(S):
            g_ids, h_ids = {}, {}
            for f, (hyps, gts) in enumerate(units[k][s]):
                for d in hyps:
                    d['e'], d['dense'] = e_d, h_ids.setdefault(d['id'], len(h_ids))
                    e_d += 1
                for j in gts:
                    j['e'], j['dense'] = e_g, g_ids.setdefault(j['id'], len(g_ids))
                    e_g += 1
                if not hyps or not gts or k * I + first[s] + f in unlisted:
                    blocks.append(None)
                elif rotated:
                    a = np.array([d['box'][:5] for d in hyps], np.float32).astype(np.float64)
                    b = np.array([j['box'][:5] for j in gts], np.float32).astype(np.float64)
                    blocks.append(np.asarray(_rotbox_ref.iou_matrix(a, b), np.float64).reshape(len(hyps), len(gts)))
                else:
                    blocks.append(np.array([[_eval_ref.iou_axis(d['box'], j['box'], False) for j in gts] for d in hyps], np.float64))
            gid_start.append(gid_start[-1] + len(g_ids))
            hid_start.append(hid_start[-1] + len(h_ids))
            ov_start.append(ov_start[-1] + len(g_ids) * len(h_ids))
    if ious is not None:
        flat, at = np.asarray(ious, np.float64), 0
        for n, b in enumerate(blocks):
            if b is not None:
                blocks[n] = flat[at:at + b.size].reshape(b.shape)
                at += b.size
        assert at == flat.size
    D, G, U, n_ov = e_d, e_g, S * K, ov_start[-1]
    block_of = iter(blocks)
    blocks = [[[next(block_of) for _ in units[k][s]] for s in range(S)] for k in range(K)]

    pot = np.zeros(n_ov, np.int64)
    gt_count, dt_count = np.zeros(gid_start[-1], np.int32), np.zeros(hid_start[-1], np.int32)
    score_q = []
    match = np.full(G, -1, np.int32)
    counts = np.zeros((U, T, 3), np.int64)
    matches = np.zeros((T, n_ov), np.int32)
    loc_sum, ass_sum = np.zeros((U, T)), np.zeros((U, T, 3))
    n_loc, n_ass = np.zeros((U, T), np.int64), np.zeros((U, T), np.int64)
    for k in range(K):
        for s in range(S):
            u = k * S + s
            n_g, n_h = gid_start[u + 1] - gid_start[u], hid_start[u + 1] - hid_start[u]
            P = pot[ov_start[u]:ov_start[u + 1]].reshape(n_g, n_h)
            gc, hc = gt_count[gid_start[u]:gid_start[u + 1]], dt_count[hid_start[u]:hid_start[u + 1]]
            part = [(hyps, gts, block) for (hyps, gts), block in zip(units[k][s], blocks[k][s]) if block is not None or not hyps or not gts]
            for hyps, gts, block in part:                                             # 1. alignment
                for j in gts:
                    gc[j['dense']] += 1
                for d in hyps:
                    hc[d['dense']] += 1
                if block is None:
                    continue
                rowsum, colsum = [0.0] * len(gts), [0.0] * len(hyps)
                for c in range(len(hyps)):
                    for r in range(len(gts)):
                        v = _value(block[c, r])
                        rowsum[r] = rowsum[r] + v                                     # over the columns, ascending
                        colsum[c] = colsum[c] + v                                     # over the rows, ascending
                for c, d in enumerate(hyps):
                    for r, j in enumerate(gts):
                        v = float(block[c, r])
                        if v > 0:
                            den = rowsum[r] + colsum[c] - v
                            sc = v / den
                            if 0.0 <= sc <= 1.0:
                                P[j['dense'], d['dense']] += math.floor(sc * 1073741824.0)
            rows = cols = 0
            tp, terms = [0] * T, [[] for _ in range(T)]
            M = matches[:, ov_start[u]:ov_start[u + 1]].reshape(T, n_g, n_h)
            for hyps, gts, block in part:                                             # 2. and 3.
                rows += len(gts)
                cols += len(hyps)
                if block is None:
                    continue
                q = pair_scores(block, [[P[j['dense'], d['dense']] for d in hyps] for j in gts], [gc[j['dense']] for j in gts],
                                [hc[d['dense']] for d in hyps])
                score_q.append(q.ravel())
                col_of_row, _ = _mot_ref.assign(Q_ONE - q.T)
                for r, c in enumerate(col_of_row):
                    if c < 0:
                        continue
                    match[gts[r]['e']] = hyps[c]['e']
                    for t, alpha in enumerate(alphas):                                # 4.
                        if block[c, r] >= alpha:                                      # NaN: False
                            tp[t] += 1
                            terms[t].append(float(block[c, r]))
                            M[t, gts[r]['dense'], hyps[c]['dense']] += 1
            for t in range(T):
                counts[u, t] = (tp[t], rows - tp[t], cols - tp[t])
                loc_sum[u, t], n_loc[u, t] = math.fsum(terms[t]), len(terms[t])
                ass = [[], [], []]
                for o in range(n_g):
                    for h in range(n_h):
                        m = int(M[t, o, h])
                        if m > 0:
                            md = float(m)
                            ass[0].append(md * (md / float(max(1, int(gc[o]) + int(hc[h]) - m))))
                            ass[1].append(md * (md / float(max(1, int(gc[o])))))
                            ass[2].append(md * (md / float(max(1, int(hc[h])))))
                ass_sum[u, t] = [math.fsum(a) for a in ass]
                n_ass[u, t] = len(ass[0])
    flat = [b.ravel() for ks in blocks for ss in ks for b in ss if b is not None]
    return {'S': S, 'K': K, 'U': U, 'D': D, 'G': G, 'seq_names': names, 'alphas': alphas,
            'ious': np.concatenate(flat) if flat else np.zeros(0), 'pot': pot, 'gt_count': gt_count, 'dt_count': dt_count,
            'score_q': (np.concatenate(score_q) if score_q else np.zeros(0, np.int64)).astype(np.int32), 'hota_match': match,
            'counts': counts, 'matches': matches, 'loc_sum': loc_sum, 'ass_sum': ass_sum, 'n_loc': n_loc, 'n_ass': n_ass,
            'gt_id_start': np.array(gid_start, np.int32), 'dt_id_start': np.array(hid_start, np.int32), 'ov_start': np.array(ov_start, np.int64)}


def summarize(r):
    """Rule 5 on the arrays of `evaluate`: {'overall': entry, 'sequences': {name: entry}}; an entry holds 'per_alpha' lists and the
    scalar means.  The sums over units are math.fsum."""
    S, K, T = r['S'], r['K'], len(r['alphas'])

    def ratio(a, b):
        return float(a) / float(b) if b else 0.0

    def entry(units):
        per = {k: [] for k in ('tp', 'fn', 'fp', 'hota', 'deta', 'assa', 'detre', 'detpr', 'assre', 'asspr', 'loca')}
        for t in range(T):
            tp, fn, fp = (int(sum(int(r['counts'][u, t, i]) for u in units)) for i in range(3))
            loc = math.fsum(r['loc_sum'][u, t] for u in units)
            ass = [math.fsum(r['ass_sum'][u, t, i] for u in units) for i in range(3)]
            deta, assa = ratio(tp, tp + fn + fp), ratio(ass[0], max(1, tp))
            for k, v in (('tp', tp), ('fn', fn), ('fp', fp), ('deta', deta), ('assa', assa), ('detre', ratio(tp, tp + fn)),
                         ('detpr', ratio(tp, tp + fp)), ('assre', ratio(ass[1], max(1, tp))), ('asspr', ratio(ass[2], max(1, tp))),
                         ('loca', loc / tp if tp else 1.0), ('hota', math.sqrt(deta * assa))):
                per[k].append(v)
        out = {'per_alpha': per}
        for k in per:
            if k not in ('tp', 'fn', 'fp'):
                out[k] = math.fsum(per[k]) / T
        out['hota0'], out['loca0'] = per['hota'][0], per['loca'][0]
        out['hota_loca0'] = out['hota0'] * out['loca0']
        return out

    return {'alphas': list(r['alphas']), 'overall': entry(list(range(S * K))),
            'sequences': {name: entry([k * S + s for k in range(K)]) for s, name in enumerate(r['seq_names'])}}
