"""Appearance in the optimal assignment: what the tracker launch on the fused IoU-and-appearance cost costs next to the launches it
stands beside (profiles/appearance_optimal.md):

    python tools/bench_appearance_optimal.py [--frames 8] [--samples 30] [--out FILE.json] [--md FILE.md]

One stream of `frames` 1080p frames per call, 20, 100 and 300 objects per frame (the records of tools/bench_track.py, rotated boxes,
`max_tracks=512`; the noise frames and the descriptors of tools/bench_appearance.py).  Every form runs call after call on its own
persistent state, as the existing benchmarks do: the scene jumps back at every call, so at 300 objects the state fills up to 512
tracks -- the worst corner of tools/bench_appearance.py.  In the same run, alternating sample by sample:

    optimal      ops.track_frames with assign='optimal' and no appearance (mydet_track_frames_assoc_f32): the yardstick
    fused        the same with appear= at weight 128 (gate 0.3, reid 0.6): mydet_track_frames_appear_optimal_f32
    phase        the fused entry point with weight 0, gate 0 and reid 0: the outputs of `optimal`, so the difference is the
                 similarity phase (and the cost functor's one load)
    greedy       the greedy appearance launch (mydet_track_frames_appear_f32, gate 0.3, reid 0.6)

`pairs` is the number of workspace words the phase wrote in one call, counted frame by frame on a workspace of sentinels.
Medians of `samples` after 3 warm-up samples between two device events.  --md writes the tables; what follows the line
`<!-- notes -->` in an existing file is kept."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from bench_appearance import HW, cell, noise_frames  # noqa: E402
from bench_motion import NOTES, timed  # noqa: E402
from bench_track import records  # noqa: E402

FORMS = ('optimal', 'fused', 'phase', 'greedy')
SENTINEL = -7


def count_pairs(ops, rec, desc, par, opt, aset, F, dev):
    """The workspace words one call writes, frame by frame (S >= 0, so a sentinel word that changed was written)."""
    state, astate, ws = ops.track_state(1, 512, dev), ops.appear_state(1, 512, dev), ops.appear_workspace(1, 512, dev)
    for _ in range(4):                                               # the state the timed calls settle into
        ops.track_frames(rec, state, par, assoc=opt, appear=(aset, desc, astate), appear_weight=128, appear_ws=ws)
    pairs = []
    for f in range(F):
        ws.fill_(SENTINEL)
        ops.track_frames(rec[f:f + 1], state, par, assoc=opt, appear=(aset, desc[f:f + 1].contiguous(), astate), appear_weight=128, appear_ws=ws)
        pairs.append(int((ws != SENTINEL).sum()))
    return pairs


def tables(r):
    F = r['frames_per_launch']
    rows = [f'| objects | live tracks | optimal, {F} frames, us | fused (weight 0.5), us | phase alone (weight 0, gate 0, reid 0), us | greedy appearance, us |',
            '|---|---|---|---|---|---|']
    for c in r['tracker']:
        rows.append(f"| {c['objects']} | {c['live_tracks']} | " + ' | '.join(cell(c[k]) for k in FORMS) + ' |')
    rows += ['', '| objects | optimal, us / frame | fused, us / frame | fused / optimal | phase share of the fused launch | pairs / call | phase, ns / pair |',
             '|---|---|---|---|---|---|---|']
    for c in r['tracker']:
        o, fu, ph = (c[k]['median_us'] for k in ('optimal', 'fused', 'phase'))
        n = sum(c['pairs'])
        per = f'{(ph - o) * 1e3 / n:.0f}' if n else '-'
        rows.append(f"| {c['objects']} | {o / F:.1f} | {fu / F:.1f} | {fu / o:.2f} | {max(ph - o, 0.0) / fu:.2f} | {n} | {per} |")
    return '\n'.join(rows)


def write_md(path, r):
    notes = ''
    if os.path.exists(path):
        old = open(path).read()
        if NOTES in old:
            notes = old.split(NOTES, 1)[1]
    head = (f"# Appearance in the optimal assignment: the tracker launch on the fused cost (one MI355X)\n\n"
            f"Command: `python tools/bench_appearance_optimal.py` (one stream of {r['frames_per_launch']} frames of {HW[0]} x {HW[1]} per call; the "
            f"records of `tools/bench_track.py`, rotated boxes, `max_tracks=512`; noise frames in 8 x 8 blocks).  Device `{r['device']}`, shader "
            f"clock {r['sclk_mhz_at_start']} MHz before the first launch and {r['sclk_mhz_at_end']} MHz after the last.  No profiler attached.  A "
            f"figure is the median of {r['samples']} samples after 3 warm-up samples (min - max in brackets), one sample = one call between two "
            f"device events, every buffer on the device and `out=` given; the four launches of a row alternate sample by sample, each on its own "
            f"persistent state.\n\n")
    with open(path, 'w') as f:
        f.write(head + tables(r) + '\n\n' + NOTES + notes)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=8)
    ap.add_argument('--samples', type=int, default=30)
    ap.add_argument('--out', default=None)
    ap.add_argument('--md', default=None)
    args = ap.parse_args()
    from mydetection_amd import ops
    assert torch.cuda.is_available(), 'bench_appearance_optimal.py measures on the MI355X; there is no CPU path'
    dev = torch.device('cuda', 0)
    F = args.frames
    r = {'device': torch.cuda.get_device_name(0), 'frames_per_launch': F, 'samples': args.samples, 'tracker': []}

    def clock():
        try:
            return torch.cuda.clock_rate()
        except Exception as e:                                       # the management library is optional
            return f'unavailable ({type(e).__name__})'
    r['sclk_mhz_at_start'] = clock()
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)
    frames = noise_frames(F, gen, dev)
    par, opt = ops.track_params(HW, 'rotated'), ops.track_assoc('optimal')
    aset, off = ops.appear_set(0.3, 0.6, 0.9, 2.0, 0.3), ops.appear_set(None, None, 0.9, 2.0, 0.3)
    for objects in (20, 100, 300):
        rec = torch.from_numpy(records(1, F, objects, 5, seed=objects + 1)).to(dev)
        desc = ops.appear_records(frames, ops.record_views(rec))
        st = {k: ops.track_state(1, 512, dev) for k in FORMS}
        ast = {k: ops.appear_state(1, 512, dev) for k in FORMS[1:]}
        ws = {k: ops.appear_workspace(1, 512, dev) for k in ('fused', 'phase')}
        calls = {'optimal': lambda out=None: ops.track_frames(rec, st['optimal'], par, assoc=opt, out=out),
                 'fused': lambda out=None: ops.track_frames(rec, st['fused'], par, assoc=opt, out=out, appear=(aset, desc, ast['fused']),
                                                            appear_weight=128, appear_ws=ws['fused']),
                 'phase': lambda out=None: ops.track_frames(rec, st['phase'], par, assoc=opt, out=out, appear=(off, desc, ast['phase']),
                                                            appear_weight=0, appear_ws=ws['phase']),
                 'greedy': lambda out=None: ops.track_frames(rec, st['greedy'], par, out=out, appear=(aset, desc, ast['greedy']))}
        outs = {k: calls[k]() for k in FORMS}
        c = {'objects': objects}
        for k, t in zip(FORMS, timed([(lambda k=k: calls[k](outs[k])) for k in FORMS], args.samples)):
            c[k] = t
        torch.cuda.synchronize()
        c['live_tracks'] = int(outs['fused']['count'][0, -1])
        c['phase_equals_optimal'] = bool(all(torch.equal(outs['phase'][k], outs['optimal'][k]) for k in outs['optimal']) and
                                         torch.equal(st['phase'], st['optimal']))
        c['matched'], c['reidentified'] = int(((outs['fused']['how'] >= 1) & (outs['fused']['how'] <= 2)).sum()), int((outs['fused']['how'] == 3).sum())
        c['pairs'] = count_pairs(ops, rec, desc, par, opt, aset, F, dev)
        print(json.dumps(c), flush=True)
        r['tracker'].append(c)
    r['sclk_mhz_at_end'] = clock()
    print(tables(r), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(r, f, indent=1)
    if args.md:
        os.makedirs(os.path.dirname(os.path.abspath(args.md)), exist_ok=True)
        write_md(args.md, r)


if __name__ == '__main__':
    main()
