"""Input stage for NV12 video, three variants alternating in one process (profiles/nv12.md):

    (a) ops.nv12_to_input                      one launch from the two planes
    (b) ops.nv12_to_rgb + ops.frames_to_input  what a user of this library had to do before: an RGB batch goes to HBM and back
    (c) ops.frames_to_input on ready-made RGB  the floor the RGB path set (the conversion is somebody else's cost)

    python tools/bench_nv12.py [--batch 16] [--height 1080] [--width 1920] [--input-size 640] [--rounds 15] [--reps 20] [--out FILE.json]

The three outputs are compared bit for bit first.  Then `rounds` alternating samples a, a', b, c (a' is a again: the spread
of two runs of the same code), each sample = `reps` back-to-back calls between two device events; medians.  The frames
rotate through enough device buffers to exceed the 256 MiB Infinity Cache, so the source comes from HBM.  Bytes per
launch are computed from the shapes (source read once, output written once); floor = those bytes / 6.3 TB/s (the
achievable HBM rate).  Also: the host-to-device bytes of one NV12 and one RGB batch and the time of that copy from
pinned memory."""
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
    ap.add_argument('--height', type=int, default=1080)
    ap.add_argument('--width', type=int, default=1920)
    ap.add_argument('--input-size', type=int, default=640)
    ap.add_argument('--rounds', type=int, default=15)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    from mydetection_amd import ops
    from mydetection_amd.api import Detector
    assert torch.cuda.is_available(), 'bench_nv12.py measures on the MI355X; there is no CPU path'
    assert args.height % 2 == 0 and args.width % 2 == 0
    dev = torch.device('cuda', 0)
    B, H, W = args.batch, args.height, args.width
    fmt = 'RGB_1_norm'
    geo = Detector._geometry(types.SimpleNamespace(divisibe=32), H, W, 'resize_pad_square', args.input_size)
    target, _, (Hp, Wp), _ = geo
    rng = np.random.Generator(np.random.PCG64(3))
    nv12_bytes, rgb_bytes, out_bytes = B * H * W * 3 // 2, B * H * W * 3, B * 3 * Hp * Wp * 4
    n_nv12, n_rgb = -(-300 * 2 ** 20 // nv12_bytes), -(-300 * 2 ** 20 // rgb_bytes)
    # single surfaces [B, H*3/2, W], as a decoder hands them over; the planes are views
    surfaces = [torch.from_numpy(rng.integers(0, 256, size=(B, H * 3 // 2, W), dtype=np.uint8)).to(dev) for _ in range(n_nv12)]
    planes = [Detector._yuv_planes(s, 'nv12') for s in surfaces]
    rgbs = [ops.nv12_to_rgb(*planes[i % n_nv12]) for i in range(n_rgb)]
    turn = [0]

    def fused():
        y, uv = planes[turn[0] % n_nv12]
        turn[0] += 1
        return ops.nv12_to_input(y, uv, geo, fmt)

    def two_step():
        y, uv = planes[turn[0] % n_nv12]
        turn[0] += 1
        return ops.frames_to_input(ops.nv12_to_rgb(y, uv), geo, fmt)

    def rgb_only():
        f = rgbs[turn[0] % n_rgb]
        turn[0] += 1
        return ops.frames_to_input(f, geo, fmt)

    outs = []
    for fn in (fused, two_step, rgb_only):
        turn[0] = 0
        outs.append(fn())
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2]), 'the three variants disagree'
    del outs

    def sample(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.reps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / args.reps              # us per call

    for fn in (fused, two_step, rgb_only):                       # warm-up: code objects, tables, allocator
        for _ in range(3):
            sample(fn)
    ta, ta2, tb, tc = [], [], [], []
    for _ in range(args.rounds):
        ta.append(sample(fused))
        ta2.append(sample(fused))
        tb.append(sample(two_step))
        tc.append(sample(rgb_only))
    ma, ma2, mb, mc = (statistics.median(t) for t in (ta, ta2, tb, tc))

    # host-to-device: one batch from pinned memory, median of 9 copies
    h2d = {}
    for name, nbytes in (('nv12', nv12_bytes), ('rgb', rgb_bytes)):
        host = torch.empty(nbytes, dtype=torch.uint8).pin_memory()
        dst = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        ts = []
        for _ in range(11):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            dst.copy_(host, non_blocking=True)
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e3)
        h2d[name] = {'bytes': nbytes, 'copy_us': round(statistics.median(ts[2:]), 1)}

    traffic = {                                                  # bytes each launch reads / writes, from the shapes
        'a_nv12_to_input': {'read': nv12_bytes, 'write': out_bytes},
        'b_nv12_to_rgb': {'read': nv12_bytes, 'write': rgb_bytes},
        'b_frames_to_input': {'read': rgb_bytes, 'write': out_bytes},
        'c_frames_to_input': {'read': rgb_bytes, 'write': out_bytes},
    }
    floor = lambda *ks: sum(traffic[k]['read'] + traffic[k]['write'] for k in ks) / HBM_BYTES_PER_S * 1e6
    fa, fb, fc = floor('a_nv12_to_input'), floor('b_nv12_to_rgb', 'b_frames_to_input'), floor('c_frames_to_input')
    r = {'frames': [B, H, W], 'resize_to': list(target), 'input': [Hp, Wp], 'buffers': [n_nv12, n_rgb],
         'a_fused_us': round(ma, 2), 'a_again_us': round(ma2, 2), 'b_convert_then_rgb_path_us': round(mb, 2), 'c_rgb_path_us': round(mc, 2),
         'a_over_b': round(ma / mb, 4), 'a_over_c': round(ma / mc, 4), 'same_code_ratio': round(ma2 / ma, 4),
         'min_us': [round(min(t), 2) for t in (ta, tb, tc)], 'max_us': [round(max(t), 2) for t in (ta, tb, tc)],
         'floor_us': [round(f, 2) for f in (fa, fb, fc)], 'over_floor': [round(m / f, 2) for m, f in ((ma, fa), (mb, fb), (mc, fc))],
         'traffic_bytes': traffic, 'h2d': h2d}
    print(json.dumps(r), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(r, f, indent=1)


if __name__ == '__main__':
    main()
