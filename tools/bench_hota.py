"""Micro-benchmark of the HOTA launches (not part of bench.py) on the sets of tools/bench_mot.py (video, frame1024, ids<N>), at the
19 default alphas, beside the CLEAR launch at the same 19 values as IoU thresholds on the same set.

--part device prints, per set, the median (and the least and largest) time over --reps samples after --warmup samples of
ops.hota_align, ops.hota_match, ops.hota_score and ops.mot_clear (HIP events on the launch stream; outputs allocated inside the
call; memsets included).  The four are sampled in turn, one sample of each per round, so that a busy neighbour hits all alike.
--part ref times the plain restatement tests/_hota_ref.py on the same seeded inputs on the host (no GPU needed).  Both parts print
the overall TPs per alpha and two checksums of the integer outputs, so that the two files can be compared.

    python tools/bench_hota.py --part device [--reps 7] [--warmup 1] [--out profiles/hota_bench.json]
    python tools/bench_hota.py --part ref [--ref-sequences 8] [--out profiles/hota_ref.json]
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
sys.path.insert(0, os.path.join(ROOT, 'tools'))

import bench_mot                                                       # noqa: E402

ALPHAS = np.arange(1, 20) / 20.0


def checks(counts, pot, match):
    """What both parts print: the overall TP per alpha, the sum of the potentials and a position-weighted sum of hota_match."""
    match = np.asarray(match, np.int64)
    return {'tp': np.asarray(counts)[:, :, 0].sum(0).tolist(), 'pot_sum': int(np.asarray(pot, np.int64).sum()),
            'match_sum': int(((match + 1) * (np.arange(len(match)) % 1000 + 1)).sum())}


def device_part(reps, warmup, n_ids):
    import torch
    from mydetection_amd import ops
    results = []
    for name, make, _ in bench_mot.sets(n_ids):
        gt, rows = make()
        pack = ops.mot_pack(rows, gt, 'coco')
        ms = ops.MotSet(pack)
        ious = ops.eval_ious(ms)
        state = {}

        def align():
            state['pot'], state['gc'], state['dc'] = ops.hota_align(ms, ious)

        def match():
            state['q'], state['match'] = ops.hota_match(ms, ious, state['pot'], state['gc'], state['dc'])

        def score():
            state['score'] = ops.hota_score(ms, ious, state['match'], state['gc'], state['dc'], ALPHAS)

        def clear():
            state['clear'] = ops.mot_clear(ms, ious, ALPHAS)

        steps = (('hota_align', align), ('hota_match', match), ('hota_score', score), ('clear', clear))
        spans = {k: [] for k, _ in steps}
        for n in range(warmup + reps):
            for k, fn in steps:
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                if n >= warmup:
                    spans[k].append((a, b))
            torch.cuda.synchronize()
        us = {k: [a.elapsed_time(b) * 1e3 for a, b in v] for k, v in spans.items()}
        counts, matches, loc_sum, ass_sum = (t.cpu().numpy() for t in state['score'])
        raw = {'counts': counts, 'loc_sum': loc_sum, 'ass_sum': ass_sum}
        overall = ops.hota_summarize(raw, pack, ALPHAS)[0]['overall']
        results.append({'set': name, 'T': len(ALPHAS), 'sequences': pack['S'], 'frames': pack['I'], 'ground_truths': pack['G'],
                        'hypotheses': pack['D'], 'pairs': pack['n_pairs'], 'listed_groups': len(pack['groups']), 'max_gt': pack['max_gt'],
                        'max_dt': pack['max_dt'], 'overlap_entries': pack['n_ov'],
                        'us_median': {k: round(float(np.median(v)), 1) for k, v in us.items()},
                        'us_min': {k: round(float(np.min(v)), 1) for k, v in us.items()},
                        'us_max': {k: round(float(np.max(v)), 1) for k, v in us.items()},
                        'hota_three_us': round(float(sum(np.median(us[k]) for k in ('hota_align', 'hota_match', 'hota_score'))), 1),
                        'hota': overall['hota'], 'deta': overall['deta'], 'assa': overall['assa'], 'loca': overall['loca'],
                        'clear_tp': state['clear'][0].cpu().numpy()[:, :, 0].sum(0).tolist(),
                        **checks(counts, state['pot'].cpu().numpy(), state['match'].cpu().numpy())})
        print(json.dumps(results[-1]), flush=True)
    return results


def ref_part(ref_sequences, n_ids):
    import _hota_ref as href
    results = []
    for name, make, _ in bench_mot.sets(n_ids):
        gt, rows = make(n_seq=ref_sequences) if name == 'video' else make()
        t0 = time.perf_counter()
        r = href.evaluate(rows, gt, 'coco', ALPHAS)
        seconds = time.perf_counter() - t0
        overall = href.summarize(r)['overall']
        results.append({'set': name, 'T': len(ALPHAS), 'sequences': r['S'], 'ground_truths': r['G'], 'hypotheses': r['D'],
                        'reference_host_s': round(seconds, 2), 'hota': overall['hota'], 'deta': overall['deta'], 'assa': overall['assa'],
                        'loca': overall['loca'], **checks(r['counts'], r['pot'], r['hota_match'])})
        print(json.dumps(results[-1]), flush=True)
    return results


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--part', choices=('device', 'ref'), default='device')
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--ref-sequences', type=int, default=8)
    ap.add_argument('--ids', type=int, default=None, help='identities a side of the identity set (default: MYDET_MOT_MAX_IDS)')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    from mydetection_amd import _lib
    n_ids = min(_lib.MOT_MAX_IDS if args.ids is None else args.ids, _lib.MOT_MAX_IDS)
    results = device_part(args.reps, args.warmup, n_ids) if args.part == 'device' else ref_part(args.ref_sequences, n_ids)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(results, f, indent=1)


if __name__ == '__main__':
    main()
