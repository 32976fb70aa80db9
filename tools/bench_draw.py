"""The overlay renderer next to the host alternative (profiles/draw.md):

    python tools/bench_draw.py [--frames 16] [--size 1080 1920] [--samples 20] [--out FILE.json]

16 frames of 1080 x 1920 on the device, 20 and 200 boxes per frame (random positions, sides 40 .. 400 pixels, three in four of
them in the frame), plain and rotated, with and without labels ('class', 'score'), into RGB frames and into NV12 planes:

    launch    one ops.draw_boxes / ops.draw_boxes_yuv420 call (one launch) on tensors that are already on the device, between
              two device events; median of `samples` after 3 warm-ups (min - max next to it).  The frames are repainted in
              place sample after sample: the work does not depend on what the pixels hold.
    tiles     the fraction of the launch's image tiles (64 x 16 pixels RGB, 128 x 16 NV12) that some box or label reaches --
              the tile test of csrc/draw.hip restated on the host -- i.e. the part of the frames the launch reads or writes
    host      what a user does today for the same RGB frames: copy to the host, PIL.ImageDraw rectangles (polygons for rotated
              boxes) frame by frame, copy back; wall clock, one sample, split into the two copies and the drawing."""
import argparse
import json
import math
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def boxes_for(B, K, H, W, rotated, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    b = np.zeros((B, K, 5), dtype=np.float32)
    b[..., 0], b[..., 1] = rng.uniform(-W / 8, W * 9 / 8, (B, K)), rng.uniform(-H / 8, H * 9 / 8, (B, K))
    b[..., 2], b[..., 3] = rng.uniform(40, 400, (B, K)), rng.uniform(40, 400, (B, K))
    if rotated:
        b[..., 4] = rng.uniform(-90, 90, (B, K))
    return b, rng.uniform(0.3, 1.0, (B, K)).astype(np.float32), rng.integers(0, 80, (B, K)).astype(np.int64)


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
    return statistics.median(out), min(out), max(out)


def tiles_touched(boxes, scores, classes, style, H, W, tw, th):
    """The fraction of tw x th tiles some box or label reaches, by the kernel's conservative test (csrc/draw.hip: draw_collect)."""
    from mydetection_amd import ops
    ht = style.thickness / 2
    nx, ny = -(-W // tw), -(-H // th)
    total = 0
    cw = ops.glyph_atlas(style.label_height).shape[2] if style.label_flags else 0
    for b in range(boxes.shape[0]):
        hit = np.zeros((ny, nx), dtype=bool)
        for k in range(boxes.shape[1]):
            cx, cy, w, h, ang = (float(v) for v in boxes[b, k])
            c, s = abs(math.cos(math.radians(ang))), abs(math.sin(math.radians(ang)))
            ex, ey = c * (w / 2 + ht) + s * (h / 2 + ht) + 1, s * (w / 2 + ht) + c * (h / 2 + ht) + 1
            x0, x1 = max(0, math.ceil((cx - ex) / tw) - 1), min(nx - 1, math.floor((cx + ex) / tw))
            y0, y1 = max(0, math.ceil((cy - ey) / th) - 1), min(ny - 1, math.floor((cy + ey) / th))
            if x0 <= x1 and y0 <= y1:
                box = np.ones((y1 - y0 + 1, x1 - x0 + 1), dtype=bool)
                if not style.fill_alpha:                             # tiles inside the outline's hole (all four corners) are not hit
                    cc, ss = math.cos(math.radians(ang)), math.sin(math.radians(ang))
                    xs, ys = np.arange(x0, x1 + 2) * tw - cx, np.arange(y0, y1 + 2) * th - cy
                    a, bb = np.abs(xs[None, :] * cc + ys[:, None] * ss), np.abs(ys[:, None] * cc - xs[None, :] * ss)
                    corner = (a < w / 2 - ht - 1) & (bb < h / 2 - ht - 1)
                    box = ~(corner[:-1, :-1] & corner[:-1, 1:] & corner[1:, :-1] & corner[1:, 1:])
                hit[y0:y1 + 1, x0:x1 + 1] |= box
            if style.label_flags:
                lw = len(ops.draw_label_text(classes[b, k], scores[b, k], None, None, style.label_flags)) * cw
                lx = min(max(math.floor(cx - w / 2 - ht), 0), max(0, W - lw))
                ly = min(max(math.floor(cy - h / 2 - ht) - style.label_height, 0), max(0, H - style.label_height))
                hit[ly // th:min(ny - 1, (ly + style.label_height - 1) // th) + 1, lx // tw:min(nx - 1, (lx + lw - 1) // tw) + 1] = True
        total += int(hit.sum())
    return total / (boxes.shape[0] * nx * ny)


def host_alternative(frames_dev, boxes, thickness):
    """Copy to the host, PIL.ImageDraw, copy back: (copy out us, draw us, copy in us) for the batch."""
    from PIL import Image, ImageDraw
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    host = frames_dev.cpu().numpy()
    t1 = time.perf_counter()
    for b in range(host.shape[0]):
        img = Image.fromarray(host[b])
        pen = ImageDraw.Draw(img)
        for cx, cy, w, h, ang in boxes[b].tolist():
            if ang == 0:
                pen.rectangle([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], outline=(255, 0, 0), width=thickness)
            else:
                c, s = math.cos(math.radians(ang)), math.sin(math.radians(ang))
                pts = [(cx + x * c - y * s, cy + x * s + y * c) for x, y in ((-w / 2, -h / 2), (w / 2, -h / 2), (w / 2, h / 2), (-w / 2, h / 2))]
                pen.line(pts + pts[:1], fill=(255, 0, 0), width=thickness)
        host[b] = np.asarray(img)
    t2 = time.perf_counter()
    frames_dev.copy_(torch.from_numpy(host))
    torch.cuda.synchronize()
    t3 = time.perf_counter()
    return (t1 - t0) * 1e6, (t2 - t1) * 1e6, (t3 - t2) * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=16)
    ap.add_argument('--size', type=int, nargs=2, default=(1080, 1920))
    ap.add_argument('--samples', type=int, default=20)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    from mydetection_amd import ops
    B, (H, W) = args.frames, args.size
    dev = torch.device('cuda')
    gen = torch.Generator().manual_seed(1)
    frames = torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, generator=gen).to(dev)
    y = torch.randint(0, 256, (B, H, W), dtype=torch.uint8, generator=gen).to(dev)
    uv = torch.randint(0, 256, (B, (H + 1) // 2, (W + 1) // 2, 2), dtype=torch.uint8, generator=gen).to(dev)
    rows = []
    for K in (20, 200):
        for rotated in (False, True):
            boxes, scores, classes = boxes_for(B, K, H, W, rotated, seed=K + rotated)
            bd, sd, cd = (torch.from_numpy(a).to(dev) for a in (boxes, scores, classes))
            for labels in ((), ('class', 'score')):
                style = ops.draw_style(thickness=3, labels=labels, label_height=24)
                row = {'boxes': K, 'rotated': rotated, 'labels': bool(labels)}
                row['rgb_us'] = timed(lambda: ops.draw_boxes(frames, bd, style, scores=sd, classes=cd), args.samples)
                row['nv12_us'] = timed(lambda: ops.draw_boxes_yuv420((y, uv), 'nv12', bd, style, scores=sd, classes=cd), args.samples)
                row['rgb_tiles'] = tiles_touched(boxes, scores, classes, style, H, W, 64, 16)
                row['nv12_tiles'] = tiles_touched(boxes, scores, classes, style, H, W, 128, 16)
                if not labels:
                    row['host_us'] = host_alternative(frames, boxes, 3)
                rows.append(row)
                print(json.dumps(row), flush=True)
    result = {'frames': B, 'size': [H, W], 'samples': args.samples, 'device': torch.cuda.get_device_name(0),
              'clock_mhz_after': getattr(torch.cuda, 'clock_rate', lambda: None)(), 'rows': rows}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(result, f, indent=1)


if __name__ == '__main__':
    main()
