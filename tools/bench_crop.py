"""The object-chip launch (profiles/crop.md):

    python tools/bench_crop.py [--frames 8] [--size 1080 1920] [--boxes 32] [--chip 128 64] [--pad 1.2] [--samples 20] [--out FILE.json]

8 frames of 1080 x 1920 on the device, 32 boxes per frame of about 300 x 150 pixels (h x w, +-20 %, centres anywhere in the
frame, so some hang over an edge), float32 chips of 128 x 64, pad 1.2, from packed RGB frames and from NV12 planes,
axis-aligned and at 30 degrees:

    launch    `reps` ops.crop_boxes / ops.crop_boxes_yuv420 calls (one launch each) into one preallocated chip buffer, on tensors
              that are already on the device, between two device events, divided by `reps`; median of `samples` after 3 warm-ups
              (min - max next to it)
    written   bytes of chips, written once: the store-side bound is this over the HBM rate
    read      bytes of source under the padded boxes' footprints (clipped to the frame), each counted once: the least a launch
              can read; the taps themselves (4 per sub-sample, 3 x 3 sub-samples at this scale) overlap and hit L2
    torch     for the record only: torch.nn.functional.grid_sample (bilinear, one sample per chip pixel, so it aliases at this
              2.8x downscale) over the same boxes on the same card, from float32 NCHW frames -- the conversion of the uint8
              frames to that form timed apart, since a user has to do it first

The NV12 chips are checked against the chips of the converted RGB frames before anything is timed."""
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

HBM_PEAK, HBM_COPY = 8.0e12, 6.29e12     # bytes / s: specification; measured float4 copy


def boxes_for(B, K, H, W, angle, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    b = np.zeros((B, K, 5), dtype=np.float32)
    b[..., 0], b[..., 1] = rng.uniform(0, W, (B, K)), rng.uniform(0, H, (B, K))
    b[..., 2], b[..., 3] = rng.uniform(120, 180, (B, K)), rng.uniform(240, 360, (B, K))
    b[..., 4] = angle
    return b


def timed(fn, samples, reps, warmup=3):
    out = []
    for i in range(warmup + samples):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        if i >= warmup:
            out.append(e0.elapsed_time(e1) * 1e3 / reps)
    return statistics.median(out), min(out), max(out)


def footprint_pixels(boxes, pad, H, W):
    """Source pixels under the padded boxes, clipped to the frame (bounding box of the rotated rectangle), summed."""
    total = 0.0
    for cx, cy, w, h, ang in boxes.reshape(-1, 5).tolist():
        c, s = abs(math.cos(math.radians(ang))), abs(math.sin(math.radians(ang)))
        ex, ey = (c * w + s * h) * pad / 2, (s * w + c * h) * pad / 2
        total += max(0.0, min(W, cx + ex) - max(0.0, cx - ex)) * max(0.0, min(H, cy + ey) - max(0.0, cy - ey))
    return total


def grid_sample_chips(frames_f, boxes, chip, pad):
    """torch's own resampler over the same boxes: [B, K, 3, ch, cw] from float32 frames [B, 3, H, W]."""
    import torch.nn.functional as F
    B, _, H, W = frames_f.shape
    K = boxes.shape[1]
    ch, cw = chip
    rad = boxes[..., 4] * (math.pi / 180)
    c, s = torch.cos(rad), torch.sin(rad)
    hw, hh = boxes[..., 2] * pad / 2, boxes[..., 3] * pad / 2
    # normalised output (u, v) in [-1, 1] -> frame pixel (cx + u*hw*c - v*hh*s, cy + u*hw*s + v*hh*c) -> normalised input
    theta = torch.stack([torch.stack([hw * c * 2 / W, -hh * s * 2 / W, boxes[..., 0] * 2 / W - 1], dim=-1),
                         torch.stack([hw * s * 2 / H, hh * c * 2 / H, boxes[..., 1] * 2 / H - 1], dim=-1)], dim=-2)
    out = []
    for b in range(B):
        grid = F.affine_grid(theta[b], (K, 3, ch, cw), align_corners=False)
        out.append(F.grid_sample(frames_f[b:b + 1].expand(K, -1, -1, -1), grid, mode='bilinear', padding_mode='zeros', align_corners=False))
    return torch.stack(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=8)
    ap.add_argument('--size', type=int, nargs=2, default=(1080, 1920))
    ap.add_argument('--boxes', type=int, default=32)
    ap.add_argument('--chip', type=int, nargs=2, default=(128, 64))
    ap.add_argument('--pad', type=float, default=1.2)
    ap.add_argument('--samples', type=int, default=20)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_crop.py measures on the MI355X: no device found')
    from mydetection_amd import ops
    B, (H, W), K, chip = args.frames, tuple(args.size), args.boxes, tuple(args.chip)
    dev = torch.device('cuda')
    gen = torch.Generator().manual_seed(1)
    y = torch.randint(0, 256, (B, H, W), dtype=torch.uint8, generator=gen).to(dev)
    uv = torch.randint(0, 256, (B, (H + 1) // 2, (W + 1) // 2, 2), dtype=torch.uint8, generator=gen).to(dev)
    frames = ops.yuv420_to_rgb((y, uv), 'nv12')                      # the RGB frames of the same pictures
    dst = torch.zeros((B, K, 3) + chip, dtype=torch.float32, device=dev)
    dst_u8 = torch.zeros((B, K) + chip + (3,), dtype=torch.uint8, device=dev)
    written = dst.numel() * 4
    rows = []
    for angle in (0.0, 30.0):
        boxes = boxes_for(B, K, H, W, angle, seed=int(angle) + 7)
        bd = torch.from_numpy(boxes).to(dev)
        kw = dict(pad=args.pad, out='input', input_format='RGB_1_norm', dst=dst)
        want = ops.crop_boxes(frames, bd, chip, **kw).clone()
        assert torch.equal(ops.crop_boxes_yuv420((y, uv), 'nv12', bd, chip, **kw), want), 'NV12 chips differ from the chips of the RGB frames'
        px = footprint_pixels(boxes, args.pad, H, W)
        row = {'angle': angle, 'written_bytes': written, 'read_bytes_rgb': px * 3, 'read_bytes_nv12': px * 1.5}
        row['rgb_us'] = timed(lambda: ops.crop_boxes(frames, bd, chip, **kw), args.samples, args.reps)
        row['nv12_us'] = timed(lambda: ops.crop_boxes_yuv420((y, uv), 'nv12', bd, chip, **kw), args.samples, args.reps)
        row['u8_rgb_us'] = timed(lambda: ops.crop_boxes(frames, bd, chip, pad=args.pad, dst=dst_u8), args.samples, args.reps)
        for key in ('rgb', 'nv12'):
            t = row[key + '_us'][0] * 1e-6
            row[key + '_written_TBps'] = written / t / 1e12
            row[key + '_read_TBps'] = row['read_bytes_' + key] / t / 1e12
            row[key + '_store_bound_us'] = written / HBM_COPY * 1e6
        row['to_float_us'] = timed(lambda: frames.permute(0, 3, 1, 2).float(), args.samples, 4)
        frames_f = frames.permute(0, 3, 1, 2).float()
        row['grid_sample_us'] = timed(lambda: grid_sample_chips(frames_f, bd, chip, args.pad), args.samples, 4)
        del frames_f
        rows.append(row)
        print(json.dumps(row), flush=True)
    result = {'frames': B, 'size': [H, W], 'boxes': K, 'chip': list(chip), 'pad': args.pad, 'samples': args.samples, 'reps': args.reps,
              'device': torch.cuda.get_device_name(0), 'clock_mhz_after': getattr(torch.cuda, 'clock_rate', lambda: None)(), 'rows': rows}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(result, f, indent=1)


if __name__ == '__main__':
    main()
