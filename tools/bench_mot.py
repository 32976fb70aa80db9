"""Micro-benchmark of the track scorer (not part of bench.py): mydet_eval_ious_f64 and the three mydet_mot_* launches on

  video       8 sequences x 1000 frames x 40 objects (a tracker-like output: jitter, misses, spurious boxes, identity changes),
              at 1 and at 19 IoU thresholds
  frame1024   one frame of 1024 ground truths against 1024 hypotheses: the largest per-frame assignment, and with 1024
              identities a side whose overlaps are all 0 or 1 also the identity assignment with the most ties
  ids         one sequence with --ids (default MYDET_MOT_MAX_IDS) identities on each side that live 24 frames each
  idsflat     --ids / 1024 frames of the frame1024 kind with no identity in two of them (only with --ids above 1024, which needs a
              library built with that MYDET_MOT_MAX_IDS: how the cap was chosen, profiles/mot.md)

--part device prints, per launch, the median time over --reps runs after --warmup runs (HIP events on the launch stream);
--part ref times the plain restatement tests/_mot_ref.py on the same seeded inputs on the host (no GPU needed; --ref-sequences
cuts the video set to its first sequences, because the restatement is slow).

    python tools/bench_mot.py --part device [--reps 11] [--warmup 2] [--out profiles/mot_bench.json]
    python tools/bench_mot.py --part ref [--ref-sequences 1] [--out profiles/mot_ref.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def video(n_seq=8, n_frames=1000, n_obj=40, seed=0):
    """(gt dict, hypothesis rows): objects drift over a 1920 x 1080 frame; a hypothesis follows its object with jitter, is missed
    5 % of the time, changes identity with probability 0.5 % a frame; one spurious box every other frame."""
    rng = np.random.default_rng(seed)
    images, anns, rows = [], [], []
    for s in range(n_seq):
        pos = rng.uniform(0, [1800, 1000], (n_obj, 2))
        vel = rng.uniform(-2, 2, (n_obj, 2))
        size = rng.uniform(40, 120, (n_obj, 2))
        label = np.arange(n_obj)
        next_label = n_obj
        for f in range(n_frames):
            img = s * n_frames + f
            images.append({'id': img, 'video_id': s, 'frame_id': f})
            pos = pos + vel
            change = rng.random(n_obj) < 0.005
            for i in np.nonzero(change)[0]:
                label[i] = next_label
                next_label += 1
            seen = rng.random(n_obj) > 0.05
            jit = rng.uniform(-0.08, 0.08, (n_obj, 2)) * size
            for i in range(n_obj):
                anns.append({'image_id': img, 'category_id': 1, 'bbox': [pos[i, 0], pos[i, 1], size[i, 0], size[i, 1]], 'track_id': i})
                if seen[i]:
                    rows.append({'image_id': img, 'category_id': 1, 'track_id': int(label[i]),
                                 'bbox': [pos[i, 0] + jit[i, 0], pos[i, 1] + jit[i, 1], size[i, 0], size[i, 1]]})
            if f % 2:
                rows.append({'image_id': img, 'category_id': 1, 'track_id': 10 ** 6 + f,
                             'bbox': [rng.uniform(0, 1800), rng.uniform(0, 1000), 80.0, 80.0]})
    return {'images': images, 'categories': [{'id': 1}], 'annotations': anns}, rows


def frame1024(seed=1, n=1024):
    rng = np.random.default_rng(seed)
    side = 32
    cell = rng.permutation(side * side)[:n]
    g = np.stack([40.0 * (cell % side), 40.0 * (cell // side)], 1) + rng.uniform(-8, 8, (n, 2))
    order = rng.permutation(n)
    h = g[order] + rng.uniform(-8, 8, (n, 2))
    anns = [{'image_id': 0, 'category_id': 1, 'bbox': [g[i, 0], g[i, 1], 30.0, 30.0], 'track_id': i} for i in range(n)]
    rows = [{'image_id': 0, 'category_id': 1, 'bbox': [h[i, 0], h[i, 1], 30.0, 30.0], 'track_id': i} for i in range(n)]
    return {'images': [{'id': 0}], 'categories': [{'id': 1}], 'annotations': anns}, rows


def ids(n_ids, seed=2, n_frames=256, life=24):
    """Every identity lives `life` frames; about n_ids * life / n_frames of them share a frame.  A hypothesis identity follows one
    ground truth for the first part of its life and its grid neighbour's for the rest, so the overlap matrix is not diagonal."""
    rng = np.random.default_rng(seed)
    start = rng.integers(0, n_frames - life, n_ids)
    turn = rng.integers(life // 3, life, n_ids)
    images, anns, rows = [{'id': f} for f in range(n_frames)], [], []
    for f in range(n_frames):
        alive = np.nonzero((start <= f) & (f < start + life))[0]
        for i in alive:
            box = [50.0 * (i % 64) + rng.uniform(-3, 3), 50.0 * (i // 64) + rng.uniform(-3, 3), 30.0, 30.0]
            anns.append({'image_id': f, 'category_id': 1, 'bbox': box, 'track_id': int(i)})
        for h in alive:
            i = h if f - start[h] < turn[h] else (h + 1) % n_ids
            rows.append({'image_id': f, 'category_id': 1, 'track_id': int(h),
                         'bbox': [50.0 * (i % 64) + rng.uniform(-3, 3), 50.0 * (i // 64) + rng.uniform(-3, 3), 30.0, 30.0]})
    return {'images': images, 'categories': [{'id': 1}], 'annotations': anns}, rows


def idsflat(n_ids):
    gt, rows = frame1024(seed=3)
    for f in range(1, n_ids // 1024):
        more_gt, more_rows = frame1024(seed=3 + f)
        gt['images'].append({'id': f})
        gt['annotations'] += [dict(a, image_id=f, track_id=a['track_id'] + 1024 * f) for a in more_gt['annotations']]
        rows += [dict(r, image_id=f, track_id=r['track_id'] + 1024 * f) for r in more_rows]
    return gt, rows


THRS19 = np.linspace(0.05, 0.95, 19)


def sets(n_ids):
    out = [('video', video, ((0.5,), THRS19)), ('frame1024', frame1024, ((0.5,),)), (f'ids{n_ids}', lambda: ids(n_ids), ((0.5,),))]
    if n_ids > 1024:
        out.append((f'ids{n_ids}flat', lambda: idsflat(n_ids), ((0.5,),)))
    return out


def device_part(reps, warmup, n_ids):
    import torch
    from mydetection_amd import ops

    def timed(fn):
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
        return out, float(np.median([a.elapsed_time(b) for a, b in spans])) * 1e3      # microseconds

    results = []
    for name, make, thr_sets in sets(n_ids):
        gt, rows = make()
        t0 = time.perf_counter()
        pack = ops.mot_pack(rows, gt, 'coco')
        t_pack = time.perf_counter() - t0
        ms = ops.MotSet(pack)
        ious, us_iou = timed(lambda: ops.eval_ious(ms))
        for thrs in thr_sets:
            clear, us_clear = timed(lambda: ops.mot_clear(ms, ious, thrs))
            overlap, us_overlap = timed(lambda: ops.mot_id_overlap(ms, ious, thrs))
            idtp, us_assign = timed(lambda: ops.mot_id_assign(ms, overlap))
            raw = {'counts': clear[0].cpu().numpy(), 'siou': clear[1].cpu().numpy(), 'present': clear[2].cpu().numpy(),
                   'matched': clear[3].cpu().numpy(), 'idtp': idtp.cpu().numpy()}
            first = ops.mot_summarize(raw, pack, thrs)[0]['overall'][len(thrs) // 2]
            results.append({'set': name, 'T': len(thrs), 'sequences': pack['S'], 'frames': pack['I'], 'ground_truths': pack['G'],
                            'hypotheses': pack['D'], 'pairs': pack['n_pairs'], 'max_gt': pack['max_gt'], 'max_dt': pack['max_dt'],
                            'max_gt_ids': pack['max_gt_ids'], 'max_dt_ids': pack['max_dt_ids'], 'overlap_entries': pack['n_ov'],
                            'pack_host_s': round(t_pack, 3), 'us': {'ious': round(us_iou, 1), 'clear': round(us_clear, 1),
                                                                    'id_overlap': round(us_overlap, 1), 'id_assign': round(us_assign, 1)},
                            'at_iou': float(thrs[len(thrs) // 2]), 'mota': first['mota'], 'idf1': first['idf1'], 'idsw': first['idsw'],
                            'tp': first['tp'], 'idtp': first['idtp']})
            print(json.dumps(results[-1]), flush=True)
    return results


def ref_part(ref_sequences, n_ids):
    import _mot_ref as ref
    results = []
    for name, make, thr_sets in sets(n_ids):
        gt, rows = make(n_seq=ref_sequences) if name == 'video' else make()
        for thrs in thr_sets:
            t0 = time.perf_counter()
            r = ref.evaluate(rows, gt, 'coco', thrs)
            results.append({'set': name, 'T': len(thrs), 'sequences': r['S'], 'ground_truths': r['G'], 'hypotheses': r['D'],
                            'reference_host_s': round(time.perf_counter() - t0, 2), 'tp': int(r['counts'][:, len(thrs) // 2, 0].sum()),
                            'idtp': int(r['idtp'][:, len(thrs) // 2].sum())})
            print(json.dumps(results[-1]), flush=True)
    return results


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--part', choices=('device', 'ref'), default='device')
    ap.add_argument('--reps', type=int, default=11)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--ref-sequences', type=int, default=1)
    ap.add_argument('--ids', type=int, default=None, help='identities a side of the identity sets (default: MYDET_MOT_MAX_IDS)')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    from mydetection_amd import _lib
    n_ids = _lib.MOT_MAX_IDS if args.ids is None else args.ids
    results = device_part(args.reps, args.warmup, n_ids) if args.part == 'device' else ref_part(args.ref_sequences, n_ids)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(results, f, indent=1)


if __name__ == '__main__':
    main()
