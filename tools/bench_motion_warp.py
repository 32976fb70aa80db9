"""Camera motion with the similarity model next to the shift model, and the tracker launch with `warp` next to `shift`
(profiles/motion_warp.md):

    python tools/bench_motion_warp.py [--frames 8] [--samples 20] [--out FILE.json] [--md FILE.md]

The frames, the ring of more than 300 MB and the timing are those of tools/bench_motion.py: crops of one smoothed-noise texture
that move by a known random shift, so every block is textured, valid and refined, and the fit runs over every block: the full
cost.  For 1080p (k = 4) and 4K (k = 8), R = 8, RGB and NV12, one stream of `frames` frames, in the same run and alternating
sample by sample:

    shift        ops.motion_frames with model 'shift' (five launches)
    similarity   ops.motion_frames with model 'similarity' (six launches: the refine stage around every block's own vector, the
                 fit, the state), with and without the inlier mask
    tracker      ops.track_frames of `frames` frames with 20 and with 300 objects: no camera motion, shift=, warp= (a = b = deg_q = 1 and s_q = 65537 in every
                 row: no part of the rule is skipped, and the tracks stay on their boxes as they do in the other two)

Medians of `samples` after 3 warm-up samples.  --md writes the table; what follows the line `<!-- notes -->` in an existing file
is kept."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from bench_motion import MARGIN, NOTES, batch, texture, timed  # noqa: E402
from bench_track import HW as TRACK_HW, records  # noqa: E402


def cell(t):
    return f"{t['median_us']:.1f} ({t['min_us']:.1f} - {t['max_us']:.1f})"


def table(r):
    F = r['frames_per_launch']
    rows = [f'| frames | format | k | blocks | shift, {F} frames, us | similarity, us | similarity + inlier mask, us | similarity - shift, us | '
            'models right |', '|---|---|---|---|---|---|---|---|---|']
    for c in r['cases']:
        rows.append(f"| {c['hw'][0]} x {c['hw'][1]} | {c['format']} | {c['k']} | {c['blocks']} | {cell(c['shift'])} | {cell(c['similarity'])} | "
                    f"{cell(c['similarity_inliers'])} | {c['similarity']['median_us'] - c['shift']['median_us']:.1f} | "
                    f"{c['models_right']} / {c['models_checked']} |")
    rows += ['', f'| tracker launch, {F} frames | no camera motion, us | shift=, us | warp=, us |', '|---|---|---|---|']
    for t in r['tracker']:
        rows.append(f"| {t['objects']} objects | {cell(t['plain'])} | {cell(t['shift'])} | {cell(t['warp'])} |")
    return '\n'.join(rows)


def write_md(path, r):
    notes = ''
    if os.path.exists(path):
        old = open(path).read()
        if NOTES in old:
            notes = old.split(NOTES, 1)[1]
    head = (f"# Camera motion: the similarity model next to the shift model (one MI355X)\n\n"
            f"Command: `python tools/bench_motion_warp.py` (one stream of {r['frames_per_launch']} frames per call, search R = 8, the frames and "
            f"the ring of `tools/bench_motion.py`; the tracker launch is `tools/bench_track.py`'s records on {TRACK_HW[0]} x {TRACK_HW[1]} "
            f"frames, `max_tracks=512`).  Device `{r['device']}`, shader clock {r['sclk_mhz_at_start']} MHz before the first launch and "
            f"{r['sclk_mhz_at_end']} MHz after the last.  No profiler attached.  A figure is the median of {r['samples']} samples after 3 "
            f"warm-up samples (min - max in brackets), one sample = one call between two device events, every buffer on the device and "
            f"`out=` given; the calls of a row alternate sample by sample.  `models right`: the frames are pure shifts, so a right "
            f"model is `a = b = 0`, `s_q = 65536`, `deg_q = 0`, `t` = the known shift.\n\n")
    with open(path, 'w') as f:
        f.write(head + table(r) + '\n\n' + NOTES + notes)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=8)
    ap.add_argument('--samples', type=int, default=20)
    ap.add_argument('--out', default=None)
    ap.add_argument('--md', default=None)
    args = ap.parse_args()
    from mydetection_amd import ops
    assert torch.cuda.is_available(), 'bench_motion_warp.py measures on the MI355X; there is no CPU path'
    dev = torch.device('cuda', 0)
    F = args.frames
    r = {'device': torch.cuda.get_device_name(0), 'frames_per_launch': F, 'samples': args.samples, 'search': 8, 'cases': [], 'tracker': []}
    try:
        r['sclk_mhz_at_start'] = torch.cuda.clock_rate()
    except Exception as e:                                           # the management library is optional
        r['sclk_mhz_at_start'] = f'unavailable ({type(e).__name__})'
    gen = torch.Generator(device=dev)
    gen.manual_seed(5)
    rng = np.random.Generator(np.random.PCG64(5))
    for hw, k in (((1080, 1920), 4), ((2160, 3840), 8)):
        H, W = hw
        sets = {'shift': ops.motion_set(k, 8), 'similarity': ops.motion_set(k, 8, model='similarity')}
        geo = ops.motion_geometry(hw, sets['shift'])
        tex = texture(H + MARGIN, W + MARGIN, 2 * k + 3, gen, dev)
        ring = -(-300 * 2 ** 20 // (F * H * W * 3))
        rgb = [batch(tex, hw, F, 4 * k, rng) for _ in range(ring)]
        for name in ('rgb', 'nv12'):
            if name == 'rgb':
                images, layout = [b for b, _ in rgb], None
            else:
                images = []
                for b, _ in rgb:
                    v = b.to(torch.int32)
                    y = ((77 * v[..., 0] + 150 * v[..., 1] + 29 * v[..., 2] + 128) >> 8).to(torch.uint8)
                    images.append((y, torch.full((F, H // 2, W // 2, 2), 128, dtype=torch.uint8, device=dev)))
                layout = 'nv12'
            states = {m: ops.motion_state(1, hw, s, dev) for m, s in sets.items()}
            outs = {'shift': ops.motion_frames(images[0], states['shift'], sets['shift'], layout=layout),
                    'similarity': ops.motion_frames(images[0], states['similarity'], sets['similarity'], layout=layout),
                    'inliers': ops.motion_frames(images[0], states['similarity'], sets['similarity'], layout=layout, inliers=True)}
            right = checked = 0
            for img, (_, true) in zip(images, rgb):                 # what the timed calls compute, against the known shifts
                ops.motion_reset_(states['similarity'], hw, sets['similarity'])
                got = ops.motion_frames(img, states['similarity'], sets['similarity'], layout=layout)['warp'][0].cpu().tolist()
                want = [[0, 0, dx << 16, dy << 16, 65536, 0, 1] if v else [0] * 7 for dx, dy, v in true]
                right += sum(g[:7] == w for g, w in zip(got, want))
                checked += len(true)
            turn = [0, 0, 0]

            def run(i, model, key, **kw):
                def fn():
                    turn[i] += 1
                    return ops.motion_frames(images[turn[i] % ring], states[model], sets[model], layout=layout, out=outs[key], **kw)
                return fn
            case = {'hw': list(hw), 'format': name, 'k': k, 'blocks': geo['nb'], 'ring_batches': ring, 'models_right': right,
                    'models_checked': checked, 'n_inliers_first_batch': outs['similarity']['warp'][0, :, 7].tolist()}
            case['shift'], case['similarity'], case['similarity_inliers'] = timed(
                [run(0, 'shift', 'shift'), run(1, 'similarity', 'similarity'), run(2, 'similarity', 'inliers', inliers=True)], args.samples)
            print(json.dumps(case), flush=True)
            r['cases'].append(case)
            del images
        del rgb, tex
        torch.cuda.empty_cache()
    par = ops.track_params(TRACK_HW, 'iou')
    row = [1, 1, 0, 0, 65537, 1, 1, 400]                             # no part of the rule is skipped, and no track is moved off its box
    for objects in (20, 300):
        rec = torch.from_numpy(records(1, F, objects, 4, seed=objects + 1)).to(dev)
        tstate = ops.track_state(1, 512, dev)
        tout = ops.track_frames(rec, tstate, par)
        shift = torch.zeros((1, F, 4), dtype=torch.int32, device=dev)
        shift[..., 2] = 1
        warp = torch.tensor(row, dtype=torch.int32, device=dev).repeat(1, F, 1)
        plain, moved, warped = timed([lambda: ops.track_frames(rec, tstate, par, out=tout),
                                      lambda: ops.track_frames(rec, tstate, par, out=tout, shift=shift),
                                      lambda: ops.track_frames(rec, tstate, par, out=tout, warp=warp)], args.samples)
        t = {'objects': objects, 'plain': plain, 'shift': moved, 'warp': warped}
        print(json.dumps(t), flush=True)
        r['tracker'].append(t)
    try:
        r['sclk_mhz_at_end'] = torch.cuda.clock_rate()
    except Exception as e:
        r['sclk_mhz_at_end'] = f'unavailable ({type(e).__name__})'
    print(table(r), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(r, f, indent=1)
    if args.md:
        os.makedirs(os.path.dirname(os.path.abspath(args.md)), exist_ok=True)
        write_md(args.md, r)


if __name__ == '__main__':
    main()
