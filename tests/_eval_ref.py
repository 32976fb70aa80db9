"""The whole detection evaluator as plain Python / numpy float64 (test code; the package never imports it).

Written from the rule text of include/mydet.h ("Scoring detections against ground truth"), not from the package's code: it takes
the JSON lists directly and does its own packing with dictionaries and Python sorts, so it checks the packer as well.  The
rotated IoU is tests/_rotbox_ref.iou_matrix on the float32-rounded rows.  `evaluate` returns every intermediate in the layout the
rules give the device arrays, so a test compares them with ==.
"""
import bisect

import numpy as np

import _rotbox_ref

IGNORE, CROWD = 1, 2
ROW = ' {:<18} {} @[ IoU={:<9} | area={:>6s} | maxDets={:>3d} ] = {:0.3f}'
LABELS = ('all', 'small', 'medium', 'large')


def default_params():
    return {'iouThrs': np.linspace(.5, .95, 10), 'recThrs': np.linspace(0, 1, 101), 'maxDets': [1, 10, 100],
            'areaRng': [[0, 1e10], [0, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e10]]}


def iou_axis(d, g, crowd):
    dx, dy, dw, dh = (float(v) for v in d[:4])
    gx, gy, gw, gh = (float(v) for v in g[:4])
    da, ga = dw * dh, gw * gh
    w = min(dx + dw, gx + gw) - max(dx, gx)
    if w <= 0:
        return 0.0
    h = min(dy + dh, gy + gh) - max(dy, gy)
    if h <= 0:
        return 0.0
    i = w * h
    u = da if crowd else da + ga - i
    return i / u


def pack(dts, gt, kind, max_det):
    """Groups in g = k*I + i order: a list of (dets, gts) per group, each det / gt a dict of the packed fields."""
    rotated = kind == 'cepdof'
    img_ids = sorted(set(im['id'] for im in gt['images']))
    cat_ids = sorted(set(c['id'] for c in gt['categories']))
    I, K = len(img_ids), len(cat_ids)
    groups = [([], []) for _ in range(I * K)]
    for n, a in enumerate(gt['annotations']):
        if a['image_id'] not in img_ids or a['category_id'] not in cat_ids:
            continue
        crowd = bool(a.get('iscrowd', 0))
        if rotated:
            area = a['area'] if 'area' in a else a['bbox'][2] * a['bbox'][3]
            ignore = bool(a.get('ignore', False)) or crowd
        else:
            area, ignore = a['area'], crowd
        g = cat_ids.index(a['category_id']) * I + img_ids.index(a['image_id'])
        groups[g][1].append({'row': n, 'box': a['bbox'], 'area': float(area), 'flags': IGNORE * ignore + CROWD * crowd})
    for n, d in enumerate(dts):
        cat = d.get('category_id', 1) if rotated else d['category_id']
        if d['image_id'] not in img_ids or cat not in cat_ids:
            continue
        g = cat_ids.index(cat) * I + img_ids.index(d['image_id'])
        area = d['area'] if 'area' in d else d['bbox'][2] * d['bbox'][3]
        groups[g][0].append({'row': n, 'box': d['bbox'], 'area': float(area), 'score': float(d['score'])})
    for g, (dets, gts) in enumerate(groups):
        dets.sort(key=lambda d: -d['score'])                               # Python's sort is stable: ties keep input order
        del dets[max_det:]
    return groups, I, K


def evaluate(dts, gt, kind, params=None, bound=1024):
    """Everything the device computes, plus stats and summary.  `bound`: the ground truths a group may hold."""
    p = default_params()
    p.update(params or {})
    thrs, recs = [float(v) for v in p['iouThrs']], [float(v) for v in p['recThrs']]
    max_dets, ranges = sorted(int(v) for v in p['maxDets']), [[float(v) for v in r] for r in p['areaRng']]
    T, R, M, A = len(thrs), len(recs), len(max_dets), len(ranges)
    rotated = kind == 'cepdof'
    groups, I, K = pack(dts, gt, kind, max_dets[-1])
    out = {'I': I, 'K': K}

    # dense numbering: detections and ground truths in group order
    d_index, g_index, dt_start, gt_start = 0, 0, [0], [0]
    for dets, gts in groups:
        for rank, d in enumerate(dets):
            d['e'], d['rank'] = d_index, rank
            d_index += 1
        for j in gts:
            j['e'] = g_index
            g_index += 1
        dt_start.append(d_index)
        gt_start.append(g_index)
    D, G = d_index, g_index
    out.update(D=D, G=G, dt_start=np.array(dt_start, np.int32), gt_start=np.array(gt_start, np.int32),
               listed=np.array([g for g, (a, b) in enumerate(groups) if a or b], np.int32),
               dt_rows=np.array([d['row'] for dets, _ in groups for d in dets], np.int64),
               gt_rows=np.array([j['row'] for _, gts in groups for j in gts], np.int64),
               dt_score=np.array([d['score'] for dets, _ in groups for d in dets], np.float64),
               dt_area=np.array([d['area'] for dets, _ in groups for d in dets], np.float64),
               gt_area=np.array([j['area'] for _, gts in groups for j in gts], np.float64),
               gt_flags=np.array([j['flags'] for _, gts in groups for j in gts], np.uint8),
               dt_rank=np.array([d['rank'] for dets, _ in groups for d in dets], np.int32))
    assert max([len(b) for _, b in groups] + [0]) <= bound, 'a group holds more ground truths than the library takes'

    # IoU of every pair, detection-major inside a group
    flat = []
    for dets, gts in groups:
        if rotated and dets and gts:
            m = _rotbox_ref.iou_matrix(np.array([d['box'][:5] for d in dets], np.float32), np.array([j['box'][:5] for j in gts], np.float32))
        for a, d in enumerate(dets):
            d['iou'] = [float(m[a, b]) if rotated else iou_axis(d['box'], j['box'], j['flags'] & CROWD) for b, j in enumerate(gts)]
            flat += d['iou']
    out['ious'] = np.array(flat, np.float64)

    # matching
    matched, ignored = np.zeros((A, D), np.uint32), np.zeros((A, D), np.uint32)
    gt_row = np.full((A, T, D), -1, np.int32)
    for dets, gts in groups:
        for a, (lo, hi) in enumerate(ranges):
            gt_ig = [bool(j['flags'] & IGNORE) or j['area'] < lo or j['area'] > hi for j in gts]
            visit = sorted(range(len(gts)), key=lambda j: gt_ig[j])
            for t, thr in enumerate(thrs):
                done = set()
                for d in dets:
                    best, m = min(thr, 1 - 1e-10), None
                    for j in visit:
                        if j in done and not gts[j]['flags'] & CROWD:
                            continue
                        if m is not None and not gt_ig[m] and gt_ig[j]:
                            break
                        if d['iou'][j] < best:
                            continue
                        best, m = d['iou'][j], j
                    if m is not None:
                        done.add(m)
                        matched[a, d['e']] |= np.uint32(1 << t)
                        gt_row[a, t, d['e']] = gts[m]['e']
                        if gt_ig[m]:
                            ignored[a, d['e']] |= np.uint32(1 << t)
                    elif d['area'] < lo or d['area'] > hi:
                        ignored[a, d['e']] |= np.uint32(1 << t)
    out.update(matched=matched, ignored=ignored, gt_row=gt_row)

    # accumulating
    precision, recall, scores = -np.ones((T, R, K, A, M)), -np.ones((T, K, A, M)), -np.ones((T, R, K, A, M))
    order, cat_start = [], [0]
    for k in range(K):
        mine = [(d, i) for i in range(I) for d in groups[k * I + i][0]]
        mine.sort(key=lambda di: (-di[0]['score'], di[1], di[0]['rank']))
        order += [d['e'] for d, _ in mine]
        cat_start.append(len(order))
        truths = [j for i in range(I) for j in groups[k * I + i][1]]
        for a, (lo, hi) in enumerate(ranges):
            npig = sum(1 for j in truths if not (j['flags'] & IGNORE or j['area'] < lo or j['area'] > hi))
            if npig == 0:
                continue
            for mi, md in enumerate(max_dets):
                kept = [d for d, _ in mine if d['rank'] < md]
                for t in range(T):
                    tp, fp, rc, pr = 0, 0, [], []
                    for d in kept:
                        hit, skip = (matched[a, d['e']] >> t) & 1, (ignored[a, d['e']] >> t) & 1
                        tp += int(hit and not skip)
                        fp += int(not hit and not skip)
                        rc.append(tp / npig)
                        pr.append(tp / (fp + tp + 2.0 ** -52))
                    for n in range(len(pr) - 2, -1, -1):
                        pr[n] = max(pr[n], pr[n + 1])
                    recall[t, k, a, mi] = rc[-1] if kept else 0.0
                    for r, need in enumerate(recs):
                        at = bisect.bisect_left(rc, need)
                        precision[t, r, k, a, mi] = pr[at] if at < len(kept) else 0.0
                        scores[t, r, k, a, mi] = kept[at]['score'] if at < len(kept) else 0.0
    out.update(precision=precision, recall=recall, scores=scores, order=np.array(order, np.int32), cat_start=np.array(cat_start, np.int32))
    out['stats'], out['summary'] = summarize(precision, recall, thrs, max_dets)
    return out


def summarize(precision, recall, thrs, max_dets, labels=LABELS):
    """The 12 stats: rows (is AP, IoU or None for all, area label, maxDets), mean over the entries > -1, -1 when none."""
    top = max_dets[2]
    rows = [(1, None, 'all', 100), (1, .5, 'all', top), (1, .75, 'all', top), (1, None, 'small', top), (1, None, 'medium', top),
            (1, None, 'large', top), (0, None, 'all', max_dets[0]), (0, None, 'all', max_dets[1]), (0, None, 'all', top),
            (0, None, 'small', top), (0, None, 'medium', top), (0, None, 'large', top)]
    stats, text = np.zeros(12), ''
    for n, (ap, iou, label, md) in enumerate(rows):
        s = precision if ap else recall
        ts = [t for t, v in enumerate(thrs) if iou is None or v == iou]
        a_sel = [a for a, v in enumerate(labels[:s.shape[-2]]) if v == label]
        m_sel = [m for m, v in enumerate(max_dets) if v == md]
        vals = s[ts][..., a_sel, :][..., m_sel] if a_sel and m_sel else np.zeros(0)
        vals = vals[vals > -1]
        stats[n] = np.mean(vals) if vals.size else -1
        span = '{:0.2f}:{:0.2f}'.format(thrs[0], thrs[-1]) if iou is None else '{:0.2f}'.format(iou)
        text += ROW.format('Average Precision' if ap else 'Average Recall', '(AP)' if ap else '(AR)', span, label, md, stats[n]) + '\n'
    return stats, text
