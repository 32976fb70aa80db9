"""The tracker's association modes, measured (profiles/track_assoc.md):

    python tools/bench_track_assoc.py [--parent-lib OLD.so --parent-copy OLD_COPY.so] [--samples 20] [--out FILE.json]
    python tools/bench_track_assoc.py --worst [--out FILE.json]

Three parts, all with HIP events around one call (records already on the device, `out=` given), medians after a warm-up:

    same      tools/bench_track.py's workload through mydet_track_frames_f32 of this build (B) and of a library built from the
              parent commit (A, --parent-lib), alternating A / B / A' in one process, sample by sample; A' is a second copy of
              the parent's library (--parent-copy), so A against A' is the run-to-run spread the A / B difference is read against
    modes     20, 100 and 300 detections per frame against as many tracks (max_tracks 512, 16 frames per launch, one stream):
              greedy, optimal, and both with score bands (high_thres 0.6, low_thres 0.3: about a third of the detections are low)
    worst     --worst: ONE launch of the optimal assignment on 512 detections against 512 live tracks of one class that all overlap
              each other (boxes 100 x 100 whose centres differ by a few pixels), next to the greedy walk on the same records.  The
              solver inserts 512 rows; an augmentation visits at most one column more than the rows inserted before it, so at most
              512 * 513 / 2 = 131 328 steps, each over 1 024 columns = 16 per lane.  Not run in a loop.
"""
import argparse
import ctypes
import json
import os
import platform
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

from bench_track import HW, records                                   # noqa: E402

OUT_KEYS = ('box', 'score', 'cls', 'id', 'missed', 'count', 'dropped')


def event_us(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3


def stats(v):
    return {'median_us': round(statistics.median(v), 1), 'min_us': round(min(v), 1), 'max_us': round(max(v), 1)}


def old_entry(path):
    from mydetection_amd import _lib
    fn = ctypes.CDLL(path).mydet_track_frames_f32
    fn.argtypes, fn.restype = _lib.SIGNATURES['mydet_track_frames_f32'], ctypes.c_int
    return fn


def part_same(args, r):
    from mydetection_amd import _lib, ops
    libs = {'B': _lib.lib().mydet_track_frames_f32}
    if args.parent_lib:
        libs = {'A': old_entry(args.parent_lib), 'B': libs['B'], 'A2': old_entry(args.parent_copy or args.parent_lib)}
    F, mt = 16, 256
    for width, match in ((4, 'iou'), (5, 'rotated')):
        for S in (1, 8):
            for objects in (20, 200):
                rec = torch.from_numpy(records(S, F, objects, width, seed=objects + S)).cuda().view(S, F, -1)
                par = ops.track_params(HW, match)
                state = ops.track_state(S, mt, 'cuda')
                out = ops.track_frames(rec, state, par)
                a = (ops._ptr(rec), rec.stride(0), rec.stride(1), S, F, width, ctypes.byref(par), mt, ops._ptr(state),
                     *[ops._ptr(out[k]) for k in OUT_KEYS], ops._stream())
                t = {k: [] for k in libs}
                for i in range(3 + args.samples):
                    for k, fn in libs.items():
                        us = event_us(lambda: _lib.check(fn(*a), 'mydet_track_frames_f32'))
                        if i >= 3:
                            t[k].append(us)
                case = {'part': 'same', 'box_width': width, 'match': match, 'streams': S, 'objects': objects,
                        'live_tracks': out['count'][:, -1].tolist(), **{k: stats(v) for k, v in t.items()}}
                print(json.dumps(case), flush=True)
                r['cases'].append(case)


def part_modes(args, r):
    from mydetection_amd import ops
    F, mt = 16, 512
    bands = dict(low_thres=0.3, high_thres=0.6, low_match_thres=0.3)
    modes = {'greedy': None, 'optimal': ops.track_assoc('optimal'), 'greedy_bands': ops.track_assoc('greedy', **bands),
             'optimal_bands': ops.track_assoc('optimal', **bands)}
    for width, match in ((4, 'iou'), (5, 'rotated')):
        for objects in (20, 100, 300):
            rec = torch.from_numpy(records(1, F, objects, width, seed=objects)).cuda().view(1, F, -1)
            par = ops.track_params(HW, match)
            case = {'part': 'modes', 'box_width': width, 'match': match, 'objects': objects}
            for name, assoc in modes.items():
                state = ops.track_state(1, mt, 'cuda')
                out = ops.track_frames(rec, state, par, assoc=assoc)
                t = [event_us(lambda: ops.track_frames(rec, state, par, out=out, assoc=assoc)) for _ in range(2 + args.mode_samples)][2:]
                case[name] = dict(stats(t), per_frame_us=round(statistics.median(t) / F, 1), live=int(out['count'][0, -1]),
                                  matched=int((out['missed'][0, -1] == 0).sum()))
            print(json.dumps(case), flush=True)
            r['cases'].append(case)


def part_worst(args, r):
    import _track_ref as ref
    from mydetection_amd import ops
    rng = np.random.Generator(np.random.PCG64(7))
    frames = []
    for f in range(2):
        c = np.stack([600 + rng.integers(-12, 13, 512), 450 + rng.integers(-12, 13, 512), np.full(512, 100), np.full(512, 100)], axis=1)
        frames.append((c.astype(np.float32), rng.permutation(np.linspace(0.4, 0.95, 512)).astype(np.float32), np.zeros(512, np.int64)))
    rec = torch.from_numpy(ref.pack_records(frames, 4)).cuda().view(1, 2, -1)
    par = ops.track_params(HW, 'iou')
    case = {'part': 'worst', 'detections': 512, 'tracks': 512}
    for name, assoc in (('greedy', None), ('optimal', ops.track_assoc('optimal'))):
        state = ops.track_state(1, 512, 'cuda')
        ops.track_frames(rec[:, :1], state, par, assoc=assoc)                       # 512 births
        out = {}
        us = event_us(lambda: out.update(ops.track_frames(rec[:, 1:], state, par, assoc=assoc)))
        case[name] = {'one_launch_us': round(us, 1), 'matched': int((out['missed'][0, 0] == 0).sum()), 'live': int(out['count'][0, 0])}
    print(json.dumps(case), flush=True)
    r['cases'].append(case)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent-lib', default=None)
    ap.add_argument('--parent-copy', default=None)
    ap.add_argument('--samples', type=int, default=20)
    ap.add_argument('--mode-samples', type=int, default=10)
    ap.add_argument('--worst', action='store_true', help='the worst case alone: one launch, nothing else in the process')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_track_assoc.py measures on the MI355X; there is no CPU path'
    r = {'device': torch.cuda.get_device_name(0), 'host': platform.node(), 'frame_hw': list(HW), 'cases': []}

    def clock():
        try:
            return torch.cuda.clock_rate()
        except Exception as e:                                       # the management library is optional
            return f'unavailable ({type(e).__name__})'
    r['sclk_mhz_at_start'] = clock()
    if args.worst:
        part_worst(args, r)
    else:
        part_same(args, r)
        part_modes(args, r)
    r['sclk_mhz_at_end'] = clock()
    print(json.dumps({k: v for k, v in r.items() if k != 'cases'}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(r, f, indent=1)


if __name__ == '__main__':
    main()
