"""The counting overlay next to the box launch of the same call (profiles/overlay.md):

    python tools/bench_overlay.py [--frames 8] [--size 1080 1920] [--samples 20] [--out FILE.json]

8 frames of 1080 x 1920 on the device, RGB frames and NV12 planes, synthetic counting outputs:

    zones     16 polygons of 16 vertices (stars over the whole frame), 16 directed lines with their ticks, every counter label
    trails    trails of 32 points (a random walk of up to 12 pixels a frame) for 20 and for 300 tracks per frame, max_tracks 512
    both      the zones case and the 300 trails in one launch

    overlay   one ops.draw_overlay / ops.draw_overlay_yuv420 call (one launch) between two device events
    boxes     one ops.draw_boxes / ops.draw_boxes_yuv420 call on the boxes of the same tracks (20 or 300 per frame, labels
              'class' and 'id'), in the same run: the samples of the two alternate, medians of `samples` after 3 warm-ups each
    trails    the ops.trails_frames launch that keeps such trails (F frames of one stream, 512 slots, 32 points)
    touched   the bytes of the image tiles (64 x 16 pixels RGB, 128 x 16 NV12) in which the overlay changed a pixel, read and
              written once, and the time a device-to-device copy of that many bytes takes at the bandwidth a copy of the whole
              batch reached in this run -- what the touched bytes alone would cost."""
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


def event_us(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3


def alternating(fns, samples, warmup=3):
    """(median, min, max) in us of each function, their samples taken in turn."""
    out = [[] for _ in fns]
    for i in range(warmup + samples):
        for k, fn in enumerate(fns):
            us = event_us(fn)
            if i >= warmup:
                out[k].append(us)
    return [(statistics.median(v), min(v), max(v)) for v in out]


def star(cx, cy, r_out, r_in, n=16):
    return [(cx + (r_out if i % 2 == 0 else r_in) * math.cos(2 * math.pi * i / n), cy + (r_out if i % 2 == 0 else r_in) * math.sin(2 * math.pi * i / n))
            for i in range(n)]


def zone_inputs(ops, B, H, W, dev, seed=1):
    rng = np.random.default_rng(seed)
    polys = [star(W * (0.125 + 0.25 * (z % 4)), H * (0.125 + 0.25 * (z // 4)), 0.17 * H, 0.09 * H) for z in range(16)]
    lines = [((W * (l + 0.5) / 16, 0.05 * H), (W * (15.5 - l) / 16, 0.95 * H)) for l in range(16)]
    zs = ops.zone_set((H, W), polys, lines)
    geo = ops.overlay_geometry(zs, None, 3)
    zout = {'occupancy': rng.integers(0, 3, (1, B, 16)), 'zone_counts': rng.integers(0, 5000, (1, B, 16, 4)), 'line_counts': rng.integers(0, 5000, (1, B, 16, 2))}
    return dict(geometry=geo, zones_out={k: torch.from_numpy(v.astype(np.int32)).to(dev) for k, v in zout.items()},
                counters=('occupancy', 'entries', 'visits'))


def track_inputs(ops, B, H, W, K, dev, MT=512, L=32, seed=2):
    """A tracker output of K live tracks per frame walking at random, and the trails of it made by ops.trails_frames itself."""
    rng = np.random.default_rng(seed + K)
    box = np.zeros((1, B + L, MT, 5), np.float32)
    pos = rng.uniform((0, 0), (W, H), (K, 2))
    for f in range(B + L):                                               # L frames ahead fill the rings
        pos = np.clip(pos + rng.uniform(-12, 12, (K, 2)), (0, 0), (W, H))
        box[0, f, :K, :2] = pos
        box[0, f, :K, 2:4] = rng.uniform(40, 200, (K, 2))
    ids = np.zeros((1, B + L, MT), np.int64)
    ids[..., :K] = np.arange(1, K + 1)
    missed = np.full((1, B + L, MT), -1, np.int32)
    missed[..., :K] = 0
    out = {'box': box, 'id': ids, 'cls': np.zeros_like(ids), 'missed': missed, 'count': np.full((1, B + L), K, np.int32)}
    out = {k: torch.from_numpy(v).to(dev) for k, v in out.items()}
    ts = ops.trail_set(L)
    state = ops.trails_state(1, MT, L, dev)
    ops.trails_frames({k: v[:, :L].contiguous() for k, v in out.items()}, state, ts)
    last = {k: v[:, L:].contiguous() for k, v in out.items()}
    keep = state.clone()
    trails = ops.trails_frames(last, state, ts)

    def relaunch():
        state.copy_(keep)
        ops.trails_frames(last, state, ts, out=trails)
    return last, trails, relaunch


def changed_tile_bytes(before, after, tw, th, bytes_per_pixel):
    """Read + write bytes of the tw x th tiles of [B,H,W(,C)] in which a byte changed."""
    diff = (before != after)
    if diff.dim() == 4:
        diff = diff.any(dim=3)
    B, H, W = diff.shape
    pad = torch.zeros((B, -(-H // th) * th, -(-W // tw) * tw), dtype=torch.bool, device=diff.device)
    pad[:, :H, :W] = diff
    tiles = pad.view(B, pad.shape[1] // th, th, pad.shape[2] // tw, tw).any(dim=4).any(dim=2)
    return int(tiles.sum()) * tw * th * bytes_per_pixel * 2, float(tiles.float().mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=8)
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
    spare = torch.empty_like(frames)
    copy_us = alternating([lambda: spare.copy_(frames)], args.samples)[0][0]
    copy_gbs = 2 * frames.numel() / copy_us / 1e3                       # read + write
    style = ops.draw_style(label_height=24)
    box_style = ops.draw_style(thickness=3, color_by='id', labels=('class', 'id'), label_height=24)
    zones = zone_inputs(ops, B, H, W, dev)
    rows = []
    for case, K in (('zones', 20), ('trails', 20), ('trails', 300), ('both', 300)):
        track, trails, relaunch = track_inputs(ops, B, H, W, K, dev)
        kw = dict(trail_thickness=3)
        if case != 'trails':
            kw.update(zones)
        if case != 'zones':
            kw.update(trails_out=trails, track_out=track)
        boxes = track['box'][0, :, :K, :4].contiguous()
        cls, ids = track['cls'][0, :, :K].contiguous(), track['id'][0, :, :K].contiguous()
        row = {'case': case, 'tracks': K}
        (row['rgb_overlay_us'], row['rgb_boxes_us']) = alternating(
            [lambda: ops.draw_overlay(frames, style, **kw), lambda: ops.draw_boxes(frames, boxes, box_style, classes=cls, ids=ids)], args.samples)
        (row['nv12_overlay_us'], row['nv12_boxes_us']) = alternating(
            [lambda: ops.draw_overlay_yuv420((y, uv), 'nv12', style, **kw),
             lambda: ops.draw_boxes_yuv420((y, uv), 'nv12', boxes, box_style, classes=cls, ids=ids)], args.samples)
        if case != 'zones':
            row['trails_frames_us'] = alternating([relaunch], args.samples)[0]
        base = torch.zeros_like(frames)
        painted = ops.draw_overlay(base.clone(), style, **kw)
        row['rgb_touched_bytes'], row['rgb_tiles'] = changed_tile_bytes(base, painted, 64, 16, 3)
        y0 = torch.zeros_like(y)
        y1, _ = ops.draw_overlay_yuv420((y0.clone(), torch.zeros_like(uv)), 'nv12', style, **kw)
        nbytes, row['nv12_tiles'] = changed_tile_bytes(y0, y1, 128, 16, 1)
        row['nv12_touched_bytes'] = nbytes * 3 // 2                      # the luma tiles and their chroma
        row['rgb_touched_us'] = row['rgb_touched_bytes'] / copy_gbs / 1e3
        row['nv12_touched_us'] = row['nv12_touched_bytes'] / copy_gbs / 1e3
        rows.append(row)
        print(json.dumps(row), flush=True)
    result = {'frames': B, 'size': [H, W], 'samples': args.samples, 'device': torch.cuda.get_device_name(0), 'copy_us': copy_us,
              'copy_gb_per_s': copy_gbs, 'rows': rows}
    print(json.dumps({'copy_us': copy_us, 'copy_gb_per_s': copy_gbs}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(result, f, indent=1)


if __name__ == '__main__':
    main()
