"""Camera motion: the estimator's launches next to the input launch of the same frames and the tracker launch of the same call
(profiles/motion.md):

    python tools/bench_motion.py [--frames 8] [--samples 20] [--out FILE.json] [--md FILE.md]

Frames are crops of one smoothed-noise texture per channel (box mean of 2k + 3 pixels: content the k x k reduction does not
alias, see profiles/motion.md) that move by a known random shift of up to half the search range per frame, so every block is
textured, valid and refined: the full cost.  Every timed call reads another batch out of a ring of
more than 300 MB, so the frames come from HBM and not from the Infinity Cache.  For 1080p (k = 4) and 4K (k = 8), R = 8, RGB and
NV12, one stream of `frames` frames:

    motion    ops.motion_frames (five launches and the workspace allocation), state and out= given, between two device events
    input     ops.frames_to_input / ops.yuv420_to_input of the same frames (resize_pad_square to 640)
    tracker   ops.track_frames of `frames` frames with 20 and with 300 objects (the records of tools/bench_track.py)

Medians of `samples` after 3 warm-up samples, the launches of a row alternating sample by sample.  --md writes the table; what
follows the line `<!-- notes -->` in an existing file is kept."""
import argparse
import json
import os
import statistics
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from bench_track import HW as TRACK_HW, records  # noqa: E402

NOTES = '<!-- notes -->'
MARGIN = 192


def event_us(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3


def timed(fns, samples, warmup=3):
    """The launches in turn, sample by sample: what disturbs one disturbs the others."""
    got = [[] for _ in fns]
    for i in range(warmup + samples):
        for v, fn in zip(got, fns):
            t = event_us(fn)
            if i >= warmup:
                v.append(t)
    return [{'median_us': round(statistics.median(v), 1), 'min_us': round(min(v), 1), 'max_us': round(max(v), 1)} for v in got]


def texture(h, w, smooth, gen, dev):
    """Uniform noise smoothed by a smooth x smooth box mean and stretched back to the full range, uint8 [h, w, 3] on the device."""
    raw = torch.randint(0, 256, (3, 1, h + smooth - 1, w + smooth - 1), generator=gen, device=dev).float()
    v = torch.nn.functional.avg_pool2d(raw, smooth, stride=1)
    v = ((v - 127.5) * (smooth / 3.0) + 127.5).clamp(0, 255)         # the mean divides the contrast by `smooth`: keep about +-3 sigma
    return v.round().to(torch.uint8)[:, 0].permute(1, 2, 0).contiguous()


def batch(tex, hw, F, reach, rng):
    """F crops that move by a random shift of at most `reach` pixels per frame: (uint8 [F,H,W,3], the true shifts)."""
    H, W = hw
    oy = ox = MARGIN // 2
    frames, shifts = [], []
    for f in range(F):
        if f:
            dx, dy = (int(v) for v in rng.integers(-reach, reach + 1, 2))
            ny, nx = oy - dy, ox - dx
            if not (0 <= ny <= MARGIN and 0 <= nx <= MARGIN):        # turn round at the texture's edge
                dx, dy = -dx, -dy
                ny, nx = oy - dy, ox - dx
            oy, ox = ny, nx
            shifts.append([dx, dy, 1])
        else:
            shifts.append([0, 0, 0])
        frames.append(tex[oy:oy + H, ox:ox + W])
    return torch.stack(frames).contiguous(), shifts


def table(r):
    F = r['frames_per_launch']
    rows = [f'| frames | format | k | blocks | motion, {F} frames, us | input launch, us | motion / input | GB/s of frame bytes | shifts right |',
            '|---|---|---|---|---|---|---|---|---|']

    def cell(t):
        return f"{t['median_us']:.1f} ({t['min_us']:.1f} - {t['max_us']:.1f})"
    for c in r['cases']:
        rows.append(f"| {c['hw'][0]} x {c['hw'][1]} | {c['format']} | {c['k']} | {c['blocks']} | {cell(c['motion'])} | {cell(c['input'])} | "
                    f"{c['motion']['median_us'] / c['input']['median_us']:.2f} | {c['frame_bytes'] / c['motion']['median_us'] / 1e3:.0f} | "
                    f"{c['shifts_right']} / {c['shifts_checked']} |")
    rows += ['', f'| tracker launch, {F} frames | us |', '|---|---|']
    for t in r['tracker']:
        rows.append(f"| {t['objects']} objects | {cell(t['tracker'])} |")
    return '\n'.join(rows)


def write_md(path, r):
    notes = ''
    if os.path.exists(path):
        old = open(path).read()
        if NOTES in old:
            notes = old.split(NOTES, 1)[1]
    head = (f"# Camera motion: the estimator next to the input launch and the tracker launch (one MI355X)\n\n"
            f"Command: `python tools/bench_motion.py` (one stream of {r['frames_per_launch']} frames per call, search R = 8, noise textures smoothed "
            f"over 2k + 3 pixels so that every block is textured and valid; the input launch is resize_pad_square to 640; the tracker launch is `tools/bench_track.py`'s records on "
            f"{TRACK_HW[0]} x {TRACK_HW[1]} frames, `max_tracks=512`).  Device `{r['device']}`, shader clock {r['sclk_mhz_at_start']} MHz before the "
            f"first launch and {r['sclk_mhz_at_end']} MHz after the last.  No profiler attached.  A figure is the median of {r['samples']} samples "
            f"after 3 warm-up samples (min - max in brackets), one sample = one call between two device events, every buffer on the "
            f"device and `out=` given; every call reads another batch of a ring of more than 300 MB, and the launches of a row "
            f"alternate sample by sample.  `motion` is the whole of `ops.motion_frames`: five launches and the workspace allocation.  "
            f"`GB/s of frame bytes` is the bytes of the frames the rules read (RGB: 3 H W; NV12: the Y plane) over the motion time: "
            f"a whole-call rate, not a kernel's.  `shifts right` compares the result with the known shift of the crops.\n\n")
    with open(path, 'w') as f:
        f.write(head + table(r) + '\n\n' + NOTES + notes)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=8)
    ap.add_argument('--samples', type=int, default=20)
    ap.add_argument('--out', default=None)
    ap.add_argument('--md', default=None)
    args = ap.parse_args()
    from mydetection_amd import ops
    from mydetection_amd.api import Detector
    assert torch.cuda.is_available(), 'bench_motion.py measures on the MI355X; there is no CPU path'
    dev = torch.device('cuda', 0)
    F, fmt = args.frames, 'RGB_1_norm'
    r = {'device': torch.cuda.get_device_name(0), 'frames_per_launch': F, 'samples': args.samples, 'search': 8,
         'cases': [], 'tracker': []}
    try:
        r['sclk_mhz_at_start'] = torch.cuda.clock_rate()
    except Exception as e:                                           # the management library is optional
        r['sclk_mhz_at_start'] = f'unavailable ({type(e).__name__})'
    gen = torch.Generator(device=dev)
    gen.manual_seed(5)
    rng = np.random.Generator(np.random.PCG64(5))
    for hw, k in (((1080, 1920), 4), ((2160, 3840), 8)):
        H, W = hw
        mset = ops.motion_set(k, 8)
        geo = ops.motion_geometry(hw, mset)
        net = Detector._geometry(types.SimpleNamespace(divisibe=32), H, W, 'resize_pad_square', 640)
        tex = texture(H + MARGIN, W + MARGIN, 2 * k + 3, gen, dev)
        ring = -(-300 * 2 ** 20 // (F * H * W * 3))
        rgb = [batch(tex, hw, F, 4 * k, rng) for _ in range(ring)]
        for name in ('rgb', 'nv12'):
            if name == 'rgb':
                images, layout, frame_bytes = [b for b, _ in rgb], None, F * H * W * 3
            else:
                images = []
                for b, _ in rgb:
                    v = b.to(torch.int32)
                    y = ((77 * v[..., 0] + 150 * v[..., 1] + 29 * v[..., 2] + 128) >> 8).to(torch.uint8)
                    images.append((y, torch.full((F, H // 2, W // 2, 2), 128, dtype=torch.uint8, device=dev)))
                layout, frame_bytes = 'nv12', F * H * W
            state = ops.motion_state(1, hw, mset, dev)
            out = ops.motion_frames(images[0], state, mset, layout=layout)
            right = checked = 0
            for img, (_, true) in zip(images, rgb):                 # what the timed calls compute, against the known shifts
                ops.motion_reset_(state, hw, mset)
                got = ops.motion_frames(img, state, mset, layout=layout)['shift'][0, :, :3].cpu().tolist()
                right += sum(g == t for g, t in zip(got, true))
                checked += len(true)
            turn = [0, 0]

            def motion():
                turn[0] += 1
                return ops.motion_frames(images[turn[0] % ring], state, mset, layout=layout, out=out)

            def to_input():
                turn[1] += 1
                img = images[turn[1] % ring]
                return ops.frames_to_input(img, net, fmt) if layout is None else ops.yuv420_to_input(img, layout, net, fmt)
            case = {'hw': list(hw), 'format': name, 'k': k, 'blocks': geo['nb'], 'ring_batches': ring, 'frame_bytes': frame_bytes,
                    'shifts_right': right, 'shifts_checked': checked, 'n_valid_first_batch': out['shift'][0, :, 3].tolist()}
            case['motion'], case['input'] = timed([motion, to_input], args.samples)
            print(json.dumps(case), flush=True)
            r['cases'].append(case)
            del images
        del rgb, tex
        torch.cuda.empty_cache()
    par = ops.track_params(TRACK_HW, 'iou')
    for objects in (20, 300):
        rec = torch.from_numpy(records(1, F, objects, 4, seed=objects + 1)).to(dev)
        tstate = ops.track_state(1, 512, dev)
        tout = ops.track_frames(rec, tstate, par)
        shift = torch.zeros((1, F, 4), dtype=torch.int32, device=dev)
        plain, moved = timed([lambda: ops.track_frames(rec, tstate, par, out=tout), lambda: ops.track_frames(rec, tstate, par, out=tout, shift=shift)],
                             args.samples)
        t = {'objects': objects, 'live_tracks': tout['count'][:, -1].tolist(), 'tracker': plain, 'tracker_with_shift_argument': moved}
        print(json.dumps(t), flush=True)
        r['tracker'].append(t)
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
