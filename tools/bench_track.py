"""Tracking across video frames: the device launch next to the host alternative (profiles/track.md):

    python tools/bench_track.py [--frames 16] [--max-tracks 256] [--samples 20] [--host-samples 1] [--out FILE.json]

Synthetic records in frame coordinates (960 x 1280): `objects` boxes on a grid that drift a pixel or two per frame with detection
noise, three classes, so that after a few frames the tracker holds about `objects` live tracks and every frame is `objects`
matches.  For S = 1 and 8 streams, about 20 and 200 tracks, 4-wide records with match 'iou' and 5-wide records with match
'rotated':

    launch    ops.track_frames on S x F records that are already on the device, between two device events; reported per frame
              (the time of the launch / F) and for F = 1 (one frame per launch: launch latency included)
    host      what a user does without the kernel: the S x F records copied to the host (one copy), then the numpy tracker
              tests/_track_ref.py in float32, frame by frame (timed on stream 0: the host walks the streams in turn); wall
              clock per frame of one stream

Medians of `samples` (host: `host-samples`) after a warm-up that also brings the tracker to its steady state."""
import argparse
import json
import os
import platform
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

HW = (960, 1280)


def records(S, F, objects, width, seed):
    """int32 [S*F, words]: per stream `objects` boxes on a grid, drifting, in a shuffled record order with distinct scores."""
    import _track_ref as ref
    rng = np.random.Generator(np.random.PCG64(seed))
    frames = []
    for s in range(S):
        cols = int(np.ceil(np.sqrt(objects * 4 / 3)))
        k = np.arange(objects)
        step = min(HW[1] // (cols + 1), HW[0] // (objects // cols + 2))
        cx, cy = (k % cols + 1) * step, (k // cols + 1) * step
        wh = rng.uniform(0.5, 0.8, (objects, 2)) * step
        ang = rng.uniform(0, 180, objects)
        vel = rng.uniform(-1.5, 1.5, (objects, 2))
        cats = rng.integers(0, 3, objects)
        for f in range(F):
            order = rng.permutation(objects)
            b = np.stack([cx + vel[:, 0] * f, cy + vel[:, 1] * f, wh[:, 0], wh[:, 1], ang + 0.5 * f], axis=1) + rng.uniform(-0.5, 0.5, (objects, 5))
            sc = rng.permutation(np.linspace(0.4, 0.95, objects))
            frames.append((b[order][:, :width].astype(np.float32), sc.astype(np.float32), cats[order]))
    return ref.pack_records(frames, width)


def timed(fn, samples, warmup=3):
    out = []
    for i in range(warmup + samples):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        if i >= warmup:
            out.append(e0.elapsed_time(e1) * 1e3)
    return {'median_us': round(statistics.median(out), 1), 'min_us': round(min(out), 1), 'max_us': round(max(out), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=16)
    ap.add_argument('--max-tracks', type=int, default=256)
    ap.add_argument('--samples', type=int, default=20)
    ap.add_argument('--host-samples', type=int, default=1)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import _track_ref as ref
    from mydetection_amd import ops
    assert torch.cuda.is_available(), 'bench_track.py measures on the MI355X; there is no CPU path'
    dev = torch.device('cuda', 0)
    F, mt = args.frames, args.max_tracks
    r = {'device': torch.cuda.get_device_name(0), 'host': platform.node(), 'frame_hw': list(HW), 'frames_per_launch': F, 'max_tracks': mt,
         'cases': []}
    try:
        r['sclk_mhz_at_start'] = torch.cuda.clock_rate()
    except Exception as e:                                           # the management library is optional
        r['sclk_mhz_at_start'] = f'unavailable ({type(e).__name__})'
    for width, match in ((4, 'iou'), (5, 'rotated')):
        for S in (1, 8):
            for objects in (20, 200):
                rec_np = records(S, F, objects, width, seed=objects + S)
                rec = torch.from_numpy(rec_np).to(dev)
                par = ops.track_params(HW, match)
                state = ops.track_state(S, mt, dev)
                v = rec.view(S, F, -1)
                out = ops.track_frames(rec, state, par)                  # steady state: the tracks of the last frame
                case = {'box_width': width, 'match': match, 'streams': S, 'objects': objects,
                        'live_tracks': out['count'][:, -1].tolist(), 'matched_last_frame': (out['missed'][:, -1] == 0).sum(1).tolist()}
                whole = timed(lambda: ops.track_frames(rec, state, par, out=out), args.samples)
                case['launch_F'] = whole
                case['launch_per_frame_us'] = round(whole['median_us'] / F, 2)
                one = {k: t[:, :1].contiguous() for k, t in out.items()}
                case['launch_one_frame'] = timed(lambda: ops.track_frames(v[:, F - 1:F], state, par, out=one), args.samples)
                # the host alternative: one copy of the records, then numpy
                torch.cuda.synchronize()
                host = []
                for _ in range(args.host_samples):
                    stream = ref.Stream(mt, ref.Params(HW, np.float32, match=match))
                    t0 = time.perf_counter()
                    h = rec.cpu().numpy().reshape(S, F, -1)
                    t1 = time.perf_counter()
                    for f in range(F):                                   # stream 0: the host walks the streams one after the other
                        stream.step(*ref.unpack_frame(h[0, f], width))
                    t2 = time.perf_counter()
                    host.append(((t1 - t0) * 1e6 / (S * F), (t2 - t1) * 1e6 / F))
                case['host_copy_per_frame_us'] = round(statistics.median(c for c, _ in host), 1)
                case['host_numpy_per_frame_us'] = round(statistics.median(n for _, n in host), 1)
                print(json.dumps(case), flush=True)
                r['cases'].append(case)
    try:
        r['sclk_mhz_at_end'] = torch.cuda.clock_rate()
    except Exception as e:
        r['sclk_mhz_at_end'] = f'unavailable ({type(e).__name__})'
    print(json.dumps(r), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(r, f, indent=1)


if __name__ == '__main__':
    main()
