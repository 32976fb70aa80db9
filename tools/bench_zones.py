"""Counting tracks in zones and across lines: the zone launch next to the tracker launch of the same call (profiles/zones.md):

    python tools/bench_zones.py [--frames 16] [--max-tracks 512] [--samples 20] [--out FILE.json] [--md FILE.md]

The tracker side is tools/bench_track.py's: synthetic 4-wide records in frame coordinates (960 x 1280), `objects` boxes on a grid
that drift a pixel or two per frame, match 'iou', so that every frame is `objects` matches against `objects` live tracks.  The
zone side reads that tracker launch's outputs: 16 polygons of 16 vertices and 16 lines spread over the frame, with and without
a 256 x 256 heat map.  For 20, 100 and 300 objects per stream and 1 and 8 streams:

    tracker   ops.track_frames on S x F records that are on the device, between two device events
    zones     ops.zones_frames on that launch's outputs, between two device events (state, heat map and out= given)

Medians of `samples` after 3 warm-up samples, the two launches alternating sample by sample; also one frame per launch (launch
latency included).  --md writes the table; what follows the line `<!-- notes -->` in an existing file is kept."""
import argparse
import json
import math
import os
import platform
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from bench_track import HW, records  # noqa: E402

NOTES = '<!-- notes -->'


def zone_geometry(seed=3):
    """16 concave 16-gons and 16 lines over the frame."""
    rng = np.random.Generator(np.random.PCG64(seed))
    H, W = HW
    polygons = []
    for _ in range(16):
        cx, cy, r_out, phase = rng.uniform(0.15 * W, 0.85 * W), rng.uniform(0.15 * H, 0.85 * H), rng.uniform(120, 320), rng.uniform(0, 1)
        polygons.append([(cx + (r_out if i % 2 == 0 else 0.45 * r_out) * math.cos(phase + math.pi * i / 8),
                          cy + (r_out if i % 2 == 0 else 0.45 * r_out) * math.sin(phase + math.pi * i / 8)) for i in range(16)])
    lines = [((rng.uniform(0, W), rng.uniform(0, H)), (rng.uniform(0, W), rng.uniform(0, H))) for _ in range(16)]
    return polygons, lines


def event_us(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3


def timed_pair(first, second, samples, warmup=3):
    """The two launches in turn, sample by sample: what disturbs one disturbs the other."""
    a, b = [], []
    for i in range(warmup + samples):
        ta, tb = event_us(first), event_us(second)
        if i >= warmup:
            a.append(ta)
            b.append(tb)

    def stats(v):
        return {'median_us': round(statistics.median(v), 1), 'min_us': round(min(v), 1), 'max_us': round(max(v), 1)}
    return stats(a), stats(b)


def table(r):
    F = r['frames_per_launch']
    rows = [f'| streams | objects | heat | tracker, {F} frames, us | zones, {F} frames, us | zones / tracker | tracker, one frame, us | zones, one frame, us |',
            '|---|---|---|---|---|---|---|---|']

    def cell(t):
        return f"{t['median_us']:.1f} ({t['min_us']:.1f} - {t['max_us']:.1f})"
    for c in r['cases']:
        rows.append(f"| {c['streams']} | {c['objects']} | {'256 x 256' if c['heat'] else 'no'} | {cell(c['tracker_F'])} | {cell(c['zones_F'])} | "
                    f"{c['zones_F']['median_us'] / c['tracker_F']['median_us']:.2f} | {cell(c['tracker_one_frame'])} | {cell(c['zones_one_frame'])} |")
    return '\n'.join(rows)


def write_md(path, r):
    notes = ''
    if os.path.exists(path):
        old = open(path).read()
        if NOTES in old:
            notes = old.split(NOTES, 1)[1]
    head = (f"# Counting tracks in zones and across lines: the zone launch next to the tracker launch (one MI355X)\n\n"
            f"Command: `python tools/bench_zones.py` ({r['frames_per_launch']} frames per launch, `max_tracks={r['max_tracks']}`, "
            f"{HW[0]} x {HW[1]} frames, 4-wide records, match `'iou'`, the synthetic records of `tools/bench_track.py`; 16 polygons of 16 "
            f"vertices and 16 lines).  Device `{r['device']}`, shader clock {r['sclk_mhz_at_start']} MHz before the first launch and "
            f"{r['sclk_mhz_at_end']} MHz after the last.  No profiler attached.  A figure is the median of {r['samples']} samples after 3 warm-up "
            f"samples (min - max in brackets), one sample = one call between two device events with every buffer on the device and "
            f"`out=` given; the tracker launch and the zone launch of a row alternate sample by sample.  `one frame` is a launch of "
            f"one frame per stream, launch latency included.  `live` tracks and the events of the measured call are in the JSON "
            f"beside this file.\n\n")
    with open(path, 'w') as f:
        f.write(head + table(r) + '\n\n' + NOTES + notes)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=16)
    ap.add_argument('--max-tracks', type=int, default=512)
    ap.add_argument('--samples', type=int, default=20)
    ap.add_argument('--out', default=None)
    ap.add_argument('--md', default=None)
    args = ap.parse_args()
    from mydetection_amd import ops
    assert torch.cuda.is_available(), 'bench_zones.py measures on the MI355X; there is no CPU path'
    dev = torch.device('cuda', 0)
    F, mt = args.frames, args.max_tracks
    polygons, lines = zone_geometry()
    r = {'device': torch.cuda.get_device_name(0), 'host': platform.node(), 'frame_hw': list(HW), 'frames_per_launch': F, 'max_tracks': mt,
         'samples': args.samples, 'polygons': len(polygons), 'vertices': 16, 'lines': len(lines), 'cases': []}
    try:
        r['sclk_mhz_at_start'] = torch.cuda.clock_rate()
    except Exception as e:                                           # the management library is optional
        r['sclk_mhz_at_start'] = f'unavailable ({type(e).__name__})'
    for S in (1, 8):
        for objects in (20, 100, 300):
            rec = torch.from_numpy(records(S, F, objects, 4, seed=objects + S)).to(dev)
            v = rec.view(S, F, -1)
            par = ops.track_params(HW, 'iou')
            for heat_hw in (None, (256, 256)):
                zs = ops.zone_set(HW, polygons, lines, heat=heat_hw)
                tstate, zstate = ops.track_state(S, mt, dev), ops.zones_state(S, mt, dev)
                heat = ops.zones_heat(S, zs, dev) if heat_hw else None
                tout = ops.track_frames(rec, tstate, par)                # steady state: the tracks of the last frame
                zout = ops.zones_frames(tout, zstate, zs, heat=heat)
                case = {'streams': S, 'objects': objects, 'heat': bool(heat_hw), 'live_tracks': tout['count'][:, -1].tolist(),
                        'matched_last_frame': (tout['missed'][:, -1] == 0).sum(1).tolist()}
                case['tracker_F'], case['zones_F'] = timed_pair(lambda: ops.track_frames(rec, tstate, par, out=tout),
                                                                lambda: ops.zones_frames(tout, zstate, zs, heat=heat, out=zout), args.samples)
                case['occupancy_last_frame'] = zout['occupancy'][:, -1].sum(1).tolist()
                case['entries'] = zout['zone_counts'][:, -1, :, 0].sum(1).tolist()
                case['crossings'] = zout['line_counts'][:, -1].sum((1, 2)).tolist()
                tone = {k: t[:, :1].contiguous() for k, t in tout.items()}
                zone_one = {k: t[:, :1].contiguous() for k, t in zout.items()}
                case['tracker_one_frame'], case['zones_one_frame'] = timed_pair(
                    lambda: ops.track_frames(v[:, F - 1:F], tstate, par, out=tone),
                    lambda: ops.zones_frames(tone, zstate, zs, heat=heat, out=zone_one), args.samples)
                print(json.dumps(case), flush=True)
                r['cases'].append(case)
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
