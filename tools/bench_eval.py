"""Micro-benchmark of the evaluator's three launches (not part of bench.py): a synthetic set of COCO-val size -- 5 000 images, 80
categories, 100 detections and about 7 ground truths per image -- and a CEPDOF-like rotated set.  Prints, per launch, the median
time over --reps runs after --warmup runs (HIP events on the launch stream), the bytes the launch has to move at least and the
time those bytes take at --hbm-tbs.  The host packer and the host summary are timed with a wall clock.

    python tools/bench_eval.py [--reps 20] [--warmup 3] [--out profiles/eval_numbers.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mydetection_amd import ops  # noqa: E402


def synthetic(kind, n_images, n_cats, dt_per_image, gt_per_image, seed=0):
    """(detection columns, ground-truth dict): about 60 % of the detections are jittered copies of a ground truth of their image."""
    rng = np.random.default_rng(seed)
    rotated = kind == 'cepdof'
    n_gt = rng.poisson(gt_per_image, n_images)
    G = int(n_gt.sum())
    g_img = np.repeat(np.arange(n_images), n_gt)
    g_cat = rng.integers(0, n_cats, G)
    wh = np.exp(rng.uniform(np.log(8), np.log(300), (G, 2)))
    xy = rng.uniform(0, 640, (G, 2))
    g_box = np.concatenate([xy, wh] + ([rng.uniform(-90, 90, (G, 1))] if rotated else []), axis=1)
    crowd = rng.random(G) < 0.02
    anns = [{'image_id': int(i), 'category_id': int(c), 'bbox': b.tolist(), 'area': float(b[2] * b[3]), 'iscrowd': int(cr)}
            for i, c, b, cr in zip(g_img, g_cat, g_box, crowd)]
    gt = {'images': [{'id': i, 'height': 640, 'width': 640} for i in range(n_images)], 'categories': [{'id': k} for k in range(n_cats)],
          'annotations': anns}
    D = n_images * dt_per_image
    d_img = np.repeat(np.arange(n_images), dt_per_image)
    first = np.concatenate([[0], np.cumsum(n_gt)])
    pick = np.minimum(first[d_img] + (rng.random(D) * np.maximum(n_gt[d_img], 1)).astype(np.int64), max(G - 1, 0))
    near = (rng.random(D) < 0.6) & (n_gt[d_img] > 0)
    d_box = np.where(near[:, None], g_box[pick] * rng.uniform(0.9, 1.1, (D, g_box.shape[1])), np.concatenate(
        [rng.uniform(0, 640, (D, 2)), np.exp(rng.uniform(np.log(8), np.log(300), (D, 2)))] + ([rng.uniform(-90, 90, (D, 1))] if rotated else []), axis=1))
    d_cat = np.where(near, g_cat[pick], rng.integers(0, n_cats, D))
    cols = {'image_id': d_img.tolist(), 'category_id': d_cat.tolist(), 'bbox': d_box, 'score': rng.random(D), 'area': d_box[:, 2] * d_box[:, 3]}
    return cols, gt


def timed(fn, reps, warmup):
    for _ in range(warmup):
        out = fn()
    spans = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        spans.append((a, b))
    torch.cuda.synchronize()
    return out, float(np.median([a.elapsed_time(b) for a, b in spans])) * 1e3          # microseconds


def run(name, kind, shape, reps, warmup, hbm_tbs):
    cols, gt = synthetic(kind, *shape)
    p = ops.EvalParams()
    t0 = time.perf_counter()
    pack = ops.eval_pack(cols, gt, kind, p.maxDets[-1])
    t_pack = time.perf_counter() - t0
    es = ops.EvalSet(pack)
    T, A, M, R, K, D, G, P = len(p.iouThrs), len(p.areaRng), len(p.maxDets), len(p.recThrs), pack['K'], pack['D'], pack['G'], pack['n_pairs']
    ious, us_iou = timed(lambda: ops.eval_ious(es), reps, warmup)
    (matched, ignored, _), us_match = timed(lambda: ops.eval_match(es, ious, p.iouThrs, p.areaRng), reps, warmup)
    (precision, recall, _), us_acc = timed(lambda: ops.eval_accumulate(es, matched, ignored, T, p.areaRng, p.maxDets, p.recThrs), reps, warmup)
    precision, recall = precision.cpu().numpy(), recall.cpu().numpy()
    t0 = time.perf_counter()
    stats, _ = ops.eval_summarize(precision, recall, p)
    t_sum = time.perf_counter() - t0
    box = 20 if kind == 'cepdof' else 32
    n_listed = len(pack['groups'])
    nbytes = {
        # boxes and flags of both sides once, the group tables of the listed groups, the IoU buffer out
        'ious': (D + G) * box + G + n_listed * 20 + P * 8,
        # the IoU buffer in, areas and flags, the tables, both masks out
        'match': P * 8 + D * 8 + G * 9 + n_listed * 20 + 2 * A * D * 4,
        # per (a, m, t): order, rank and both masks of every detection, twice (forward and backward); the three arrays out
        'accumulate': A * M * T * D * 2 * 16 + A * M * T * G * 9 + (2 * R + 1) * T * K * A * M * 8,
    }
    out = {'set': name, 'kind': kind, 'images': pack['I'], 'categories': K, 'detections': D, 'ground_truths': G, 'pairs': P,
           'listed_groups': n_listed, 'pack_host_s': round(t_pack, 3), 'summarize_host_s': round(t_sum, 4), 'AP': float(stats[0]),
           'AP50': float(stats[1])}
    for key, us in (('ious', us_iou), ('match', us_match), ('accumulate', us_acc)):
        out[key] = {'us': round(us, 1), 'bytes': int(nbytes[key]), 'bound_us': round(nbytes[key] / (hbm_tbs * 1e6), 2)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--hbm-tbs', type=float, default=8.0, help='memory rate the byte bound is priced at, TB/s')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    results = [run('coco-val-size', 'coco', (5000, 80, 100, 7), args.reps, args.warmup, args.hbm_tbs),
               run('cepdof-like', 'cepdof', (2000, 1, 40, 12), args.reps, args.warmup, args.hbm_tbs)]
    for r in results:
        print(json.dumps(r))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(results, f, indent=1)


if __name__ == '__main__':
    main()
