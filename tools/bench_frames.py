"""Input stage alone, A/B in one process: the two-kernel path of Detector.preprocess_batch (a zero uint8 batch, one
mydet_resize_bilinear_u8 launch per frame, one mydet_preprocess_u8_f32) against the single mydet_frames_to_input_f32 launch
of Detector.predict_frames, frames already on the device.  (profiles/frames.md)

    python tools/bench_frames.py [--batch 16] [--input-size 640] [--rounds 15] [--reps 20] [--out FILE.json]

Per case: both outputs compared bit for bit first; then `rounds` alternating samples A, A', B (A' is A again: the spread of
two runs of the same code), each sample = `reps` back-to-back calls between two device events.  The frames rotate through
enough buffers to exceed the 256 MiB Infinity Cache, so the source is read from HBM.  Floor = (source bytes + float32
output bytes) / 6.3 TB/s (the achievable HBM rate)."""
import argparse
import json
import os
import statistics
import sys
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_BYTES_PER_S = 6.3e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--input-size', type=int, default=640)
    ap.add_argument('--rounds', type=int, default=15)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    from mydetection_amd import ops
    from mydetection_amd.api import Detector
    assert torch.cuda.is_available(), 'bench_frames.py measures on the MI355X; there is no CPU path'
    dev = torch.device('cuda', 0)
    geometry = types.SimpleNamespace(divisibe=32)
    rng = np.random.Generator(np.random.PCG64(3))
    fmt = 'RGB_1_norm'
    results = []
    for (H, W) in ((1080, 1920), (480, 640)):
        frame_bytes = args.batch * H * W * 3
        nbuf = min(24, -(-300 * 2 ** 20 // frame_bytes))
        bufs = [torch.from_numpy(rng.integers(0, 256, size=(args.batch, H, W, 3), dtype=np.uint8)).to(dev) for _ in range(nbuf)]
        for pre in ('resize_pad_square', 'resize_pad_divisible'):
            geo = Detector._geometry(geometry, H, W, pre, args.input_size)
            target, (top, left), (Hp, Wp), _ = geo
            turn = [0]

            def two_launch():
                f = bufs[turn[0] % nbuf]
                turn[0] += 1
                buf = torch.zeros((args.batch, Hp, Wp, 3), dtype=torch.uint8, device=dev)
                for n in range(args.batch):
                    ops.resize_bilinear_u8(f[n], target, buf[n], top, left)
                return ops.preprocess_u8(buf, (Hp, Wp), fmt)

            def fused():
                f = bufs[turn[0] % nbuf]
                turn[0] += 1
                return ops.frames_to_input(f, geo, fmt)

            turn[0] = 0
            a = two_launch()
            turn[0] = 0
            b = fused()
            assert torch.equal(a, b), 'the fused launch and the two-kernel path disagree'
            del a, b

            def sample(fn):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.reps):
                    fn()
                e1.record()
                e1.synchronize()
                return e0.elapsed_time(e1) * 1e3 / args.reps          # us per call

            for fn in (two_launch, fused):                           # warm-up: code objects, tables, allocator
                for _ in range(3):
                    sample(fn)
            ta, ta2, tb = [], [], []
            for _ in range(args.rounds):
                ta.append(sample(two_launch))
                ta2.append(sample(two_launch))
                tb.append(sample(fused))
            ma, ma2, mb = statistics.median(ta), statistics.median(ta2), statistics.median(tb)
            floor_us = (frame_bytes + args.batch * 3 * Hp * Wp * 4) / HBM_BYTES_PER_S * 1e6
            r = {'frames': [args.batch, H, W], 'preprocessing': pre, 'resize_to': list(target), 'input': [Hp, Wp], 'buffers': nbuf,
                 'two_launch_us': round(ma, 2), 'two_launch_again_us': round(ma2, 2), 'fused_us': round(mb, 2),
                 'fused_over_two_launch': round(mb / ma, 4), 'same_code_ratio': round(ma2 / ma, 4), 'floor_us': round(floor_us, 2),
                 'two_launch_over_floor': round(ma / floor_us, 2), 'fused_over_floor': round(mb / floor_us, 2),
                 'floor_fraction_fused': round(floor_us / mb, 3), 'min_us': [round(min(ta), 2), round(min(tb), 2)],
                 'max_us': [round(max(ta), 2), round(max(tb), 2)]}
            results.append(r)
            print(json.dumps(r), flush=True)
        del bufs
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(results, f, indent=1)


if __name__ == '__main__':
    main()
