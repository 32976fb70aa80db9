"""The redaction next to the overlay renderer and next to its own byte bound (profiles/redact.md):

    python tools/bench_redact.py [--frames 8] [--size 1080 1920] [--samples 20] [--out FILE.json] [--md FILE.md]

8 frames of 1080 x 1920 on the device, as RGB and as NV12; 8, 32 and 256 boxes per frame of 300 x 150 pixels (centres anywhere in
the frame), axis-aligned and at 30 degrees; 'mosaic' and 'smooth' at cell 8, 22 and 64, 'solid' once (it has no cells):

    redact    one ops.redact_boxes / ops.redact_boxes_yuv420 call -- the means kernel and the paint kernel -- on tensors that are
              already on the device, `calls` of them back to back between two device events, per call; median of `samples` after
              3 warm-ups.  The frames are redacted in place call after call: the work does not depend on what the pixels hold.
    draw      one ops.draw_boxes / ops.draw_boxes_yuv420 call with the style of api.Draw(fill_alpha=255) on the same boxes,
              measured the same way in the same run.
    bound     the bytes the redaction cannot avoid over 6.3 TB/s (the HBM rate a streaming kernel reaches on this chip): the
              pixels of every block of cells the means kernel reads (its own block test, restated on the host; none for
              'solid'), read once, plus every covered pixel, written once.  3 bytes per pixel RGB, 1.5 NV12.
    ratio     redact / bound."""
import argparse
import json
import math
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_US = 6.3e6          # 6.3 TB/s


def boxes_for(B, K, H, W, degrees, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    b = np.zeros((B, K, 5), dtype=np.float32)
    b[..., 0], b[..., 1] = rng.uniform(0, W, (B, K)), rng.uniform(0, H, (B, K))
    b[..., 2], b[..., 3], b[..., 4] = 300.0, 150.0, degrees
    return b, rng.uniform(0.3, 1.0, (B, K)).astype(np.float32), rng.integers(0, 80, (B, K)).astype(np.int64)


def timed(fn, samples, calls=10, warmup=3):
    out = []
    for i in range(warmup + samples):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        e1.synchronize()
        if i >= warmup:
            out.append(e0.elapsed_time(e1) * 1e3 / calls)
    return statistics.median(out), min(out), max(out)


def covered_pixels(boxes, H, W, pad=1.0):
    """Covered pixels of the batch ('box' shape), each counted once per frame: float64 coverage inside every row's bounding box."""
    total = 0
    for b in range(boxes.shape[0]):
        mask = np.zeros((H, W), dtype=bool)
        for cx, cy, w, h, ang in boxes[b].tolist():
            c, s = math.cos(math.radians(ang)), math.sin(math.radians(ang))
            ra, rb = w / 2 * pad, h / 2 * pad
            ex, ey = abs(c) * ra + abs(s) * rb + 1, abs(s) * ra + abs(c) * rb + 1
            x0, x1, y0, y1 = max(0, int(cx - ex)), min(W, int(cx + ex) + 1), max(0, int(cy - ey)), min(H, int(cy + ey) + 1)
            if x0 >= x1 or y0 >= y1:
                continue
            dx, dy = (np.arange(x0, x1) + 0.5 - cx)[None, :], (np.arange(y0, y1) + 0.5 - cy)[:, None]
            mask[y0:y1, x0:x1] |= (np.abs(dx * c + dy * s) <= ra) & (np.abs(dy * c - dx * s) <= rb)
        total += int(mask.sum())
    return total


def block_pixels(boxes, H, W, cell, smooth, pad=1.0):
    """Pixels of the blocks of cells the means kernel reads (csrc/redact.hip: redact_check's block shape, redact_means_kernel's test)."""
    gi, gj = -(-16 // cell), -(-64 // cell)
    if (gj * cell) % 4:
        gj += 1
    bh, bw, d = gi * cell, gj * cell, cell if smooth else 0
    ny, nx = -(-H // bh), -(-W // bw)
    rows = np.minimum(H, (np.arange(ny) + 1) * bh) - np.arange(ny) * bh
    cols = np.minimum(W, (np.arange(nx) + 1) * bw) - np.arange(nx) * bw
    total = 0
    for b in range(boxes.shape[0]):
        hit = np.zeros((ny, nx), dtype=bool)
        for cx, cy, w, h, ang in boxes[b].tolist():
            c, s = abs(math.cos(math.radians(ang))), abs(math.sin(math.radians(ang)))
            ra, rb = w / 2 * pad, h / 2 * pad
            ex, ey = c * ra + s * rb + 1, s * ra + c * rb + 1
            x0, x1 = max(0, math.ceil((cx - ex - d) / bw - 1)), min(nx - 1, math.floor((cx + ex + d) / bw))
            y0, y1 = max(0, math.ceil((cy - ey - d) / bh - 1)), min(ny - 1, math.floor((cy + ey + d) / bh))
            if x0 <= x1 and y0 <= y1:
                hit[y0:y1 + 1, x0:x1 + 1] = True
        total += int((hit * rows[:, None] * cols[None, :]).sum())
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=8)
    ap.add_argument('--size', type=int, nargs=2, default=(1080, 1920))
    ap.add_argument('--samples', type=int, default=20)
    ap.add_argument('--out', default=None)
    ap.add_argument('--md', default=None)
    args = ap.parse_args()
    from mydetection_amd import ops
    from mydetection_amd.api import Draw
    B, (H, W) = args.frames, args.size
    dev = torch.device('cuda')
    gen = torch.Generator().manual_seed(1)
    frames = torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, generator=gen).to(dev)
    y = torch.randint(0, 256, (B, H, W), dtype=torch.uint8, generator=gen).to(dev)
    uv = torch.randint(0, 256, (B, (H + 1) // 2, (W + 1) // 2, 2), dtype=torch.uint8, generator=gen).to(dev)
    draw_style = Draw(fill_alpha=255).style((H, W))
    rows = []
    for K in (8, 32, 256):
        for degrees in (0.0, 30.0):
            boxes, scores, classes = boxes_for(B, K, H, W, degrees, seed=K + int(degrees))
            bd, sd, cd = (torch.from_numpy(a).to(dev) for a in (boxes, scores, classes))
            covered = covered_pixels(boxes, H, W)
            draw_rgb = timed(lambda: ops.draw_boxes(frames, bd, draw_style, scores=sd, classes=cd), args.samples)
            draw_nv12 = timed(lambda: ops.draw_boxes_yuv420((y, uv), 'nv12', bd, draw_style, scores=sd, classes=cd), args.samples)
            for mode, cells in (('mosaic', (8, 22, 64)), ('smooth', (8, 22, 64)), ('solid', (22,))):
                for cell in cells:
                    style = ops.redact_style(mode, cell)
                    read = 0 if mode == 'solid' else block_pixels(boxes, H, W, cell, mode == 'smooth')
                    row = {'boxes': K, 'degrees': degrees, 'mode': mode, 'cell': cell, 'covered_share': covered / (B * H * W),
                           'read_share': read / (B * H * W)}
                    row['rgb_us'] = timed(lambda: ops.redact_boxes(frames, bd, style), args.samples)
                    row['nv12_us'] = timed(lambda: ops.redact_boxes_yuv420((y, uv), 'nv12', bd, style), args.samples)
                    row['draw_rgb_us'], row['draw_nv12_us'] = draw_rgb, draw_nv12
                    row['rgb_bound_us'] = 3.0 * (read + covered) / HBM_BYTES_PER_US
                    row['nv12_bound_us'] = 1.5 * (read + covered) / HBM_BYTES_PER_US
                    row['rgb_ratio'], row['nv12_ratio'] = row['rgb_us'][0] / row['rgb_bound_us'], row['nv12_us'][0] / row['nv12_bound_us']
                    rows.append(row)
                    print(json.dumps(row), flush=True)
    result = {'frames': B, 'size': [H, W], 'samples': args.samples, 'device': torch.cuda.get_device_name(0), 'rows': rows}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(result, f, indent=1)
    if args.md:
        lines = ['| boxes | deg | mode | cell | covered | read | RGB us | bound | ratio | draw RGB us | NV12 us | bound | ratio | draw NV12 us |',
                 '|---|---|---|---|---|---|---|---|---|---|---|---|---|---|']
        for r in rows:
            lines.append(f"| {r['boxes']} | {r['degrees']:.0f} | {r['mode']} | {r['cell']} | {100 * r['covered_share']:.1f} % | {100 * r['read_share']:.1f} % | "
                         f"{r['rgb_us'][0]:.1f} | {r['rgb_bound_us']:.1f} | {r['rgb_ratio']:.1f} | {r['draw_rgb_us'][0]:.1f} | "
                         f"{r['nv12_us'][0]:.1f} | {r['nv12_bound_us']:.1f} | {r['nv12_ratio']:.1f} | {r['draw_nv12_us'][0]:.1f} |")
        with open(args.md, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
