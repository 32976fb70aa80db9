"""Input stage for 4:2:0 video in the layouts beside NV12, variants alternating in one process (profiles/yuv420.md):

    (n) ops.nv12_to_input on NV12 frames                 the launch every layout is held to
    per layout (nv21, i420, p010, i010):
    (a) ops.yuv420_to_input                              one launch from the planes as the decoder stores them
    (b) repack to NV12 with torch ops + ops.nv12_to_input    what a user had to do before (10-bit: including the reduction)
    (c) ops.nv12_to_input on the repacked frames         (b) without the repack

    python tools/bench_yuv420.py [--batch 16] [--height 1080] [--width 1920] [--input-size 640] [--rounds 15] [--reps 20] [--out FILE.json]

The method is tools/bench_nv12.py's: (a), (b) and (c) of a layout are compared bit for bit first; then `rounds` alternating
samples n, n', and a, b, c of every layout (n' is n again: the spread of two runs of the same code), each sample = `reps`
back-to-back calls between two device events; medians.  The frames rotate through enough device buffers to exceed the
256 MiB Infinity Cache, so the source comes from HBM.  Bytes per launch are computed from the shapes (source read once,
output written once); the torch repack of (b) moves at least the bytes listed (its intermediates are not counted).
ops.nv12_to_input is ops.yuv420_to_input with layout 'nv12', so (n) takes the Python path and the C entry point of (a): the
two differ in the kernel instance and the bytes read alone."""
import argparse
import json
import os
import statistics
import sys
import types

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

LAYOUTS = ('nv21', 'i420', 'p010', 'i010')


def reduce10(words, layout):
    """16-bit words on the device -> uint8 by the rule of include/mydet.h, with torch ops."""
    w = words.to(torch.int32) & 0xFFFF
    v10 = (w >> 6) if layout == 'p010' else (w & 1023)
    return ((v10 + 2) >> 2).clamp_(max=255).to(torch.uint8)


def repack(planes, layout):
    """The planes of `layout` as NV12 planes, with torch ops on the device."""
    if layout == 'nv21':
        return planes[0], planes[1].flip(-1)
    if layout == 'i420':
        return planes[0], torch.stack((planes[1], planes[2]), dim=-1)
    if layout == 'p010':
        return reduce10(planes[0], layout), reduce10(planes[1], layout)
    return reduce10(planes[0], layout), torch.stack((reduce10(planes[1], layout), reduce10(planes[2], layout)), dim=-1)


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
    assert torch.cuda.is_available(), 'bench_yuv420.py measures on the MI355X; there is no CPU path'
    assert args.height % 2 == 0 and args.width % 2 == 0
    dev = torch.device('cuda', 0)
    B, H, W = args.batch, args.height, args.width
    fmt = 'RGB_1_norm'
    geo = Detector._geometry(types.SimpleNamespace(divisibe=32), H, W, 'resize_pad_square', args.input_size)
    target, _, (Hp, Wp), _ = geo
    gen = torch.Generator(device=dev).manual_seed(3)
    out_bytes, nv12_bytes = B * 3 * Hp * Wp * 4, B * H * W * 3 // 2

    def surfaces(layout):
        """Single decoder surfaces [B, H*3/2, W] of random samples, enough of them to exceed the Infinity Cache, as plane views."""
        bps = ops.yuv420_layout(layout)[1]
        n = -(-300 * 2 ** 20 // (nv12_bytes * bps))
        if bps == 1:
            raw = [torch.randint(0, 256, (B, H * 3 // 2, W), dtype=torch.uint8, device=dev, generator=gen) for _ in range(n)]
        else:
            raw = [torch.randint(-32768, 32768, (B, H * 3 // 2, W), dtype=torch.int16, device=dev, generator=gen) for _ in range(n)]
        return [tuple(Detector._yuv_planes(s, layout)) for s in raw]

    turn = [0]

    def rotating(bufs, fn):
        def call():
            p = bufs[turn[0] % len(bufs)]
            turn[0] += 1
            return fn(p)
        return call

    nv12 = surfaces('nv12')
    variants = {'n': rotating(nv12, lambda p: ops.nv12_to_input(p[0], p[1], geo, fmt))}
    variants['n_again'] = variants['n']
    traffic = {'n': {'read': nv12_bytes, 'write': out_bytes}}
    buffers = {'nv12': len(nv12)}
    for layout in LAYOUTS:
        src = surfaces(layout)
        packed = [tuple(t.contiguous() for t in repack(p, layout)) for p in src]
        buffers[layout] = len(src)
        variants[layout + '_a'] = rotating(src, lambda p, layout=layout: ops.yuv420_to_input(p, layout, geo, fmt))
        variants[layout + '_b'] = rotating(src, lambda p, layout=layout: ops.nv12_to_input(*repack(p, layout), geo, fmt))
        variants[layout + '_c'] = rotating(packed, lambda p: ops.nv12_to_input(p[0], p[1], geo, fmt))
        outs = []
        for k in 'abc':
            turn[0] = 0
            outs.append(variants[f'{layout}_{k}']())
        assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2]), f'{layout}: the three variants disagree'
        del outs
        src_bytes = nv12_bytes * ops.yuv420_layout(layout)[1]
        eight = layout in ('nv21', 'i420')                                       # 8-bit: only the chroma is rewritten, Y is used in place
        repack_read, repack_write = (nv12_bytes // 3,) * 2 if eight else (src_bytes, nv12_bytes)
        traffic[layout] = {'a': {'read': src_bytes, 'write': out_bytes},
                           'b_repack_at_least': {'read': repack_read, 'write': repack_write},
                           'b_nv12_to_input': {'read': nv12_bytes, 'write': out_bytes},
                           'c': {'read': nv12_bytes, 'write': out_bytes}}

    def sample(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.reps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / args.reps              # us per call

    for fn in variants.values():                                 # warm-up: code objects, tables, allocator
        for _ in range(3):
            sample(fn)
    times = {k: [] for k in variants}
    for _ in range(args.rounds):
        for k, fn in variants.items():
            times[k].append(sample(fn))
    med = {k: statistics.median(t) for k, t in times.items()}
    spread = abs(med['n_again'] / med['n'] - 1.0)
    r = {'frames': [B, H, W], 'resize_to': list(target), 'input': [Hp, Wp], 'buffers': buffers,
         'median_us': {k: round(v, 2) for k, v in med.items()},
         'min_us': {k: round(min(t), 2) for k, t in times.items()}, 'max_us': {k: round(max(t), 2) for k, t in times.items()},
         'same_code_ratio': round(med['n_again'] / med['n'], 4),
         'a_over_b': {la: round(med[la + '_a'] / med[la + '_b'], 4) for la in LAYOUTS},
         'a_over_c': {la: round(med[la + '_a'] / med[la + '_c'], 4) for la in LAYOUTS},
         'a_over_n': {la: round(med[la + '_a'] / med['n'], 4) for la in LAYOUTS},
         'a_faster_than_b_by_more_than_twice_the_spread': {la: bool(med[la + '_a'] < med[la + '_b'] * (1.0 - 2.0 * spread)) for la in LAYOUTS},
         'traffic_bytes': traffic}
    print(json.dumps(r), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(r, f, indent=1)


if __name__ == '__main__':
    main()
