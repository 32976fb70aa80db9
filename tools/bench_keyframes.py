"""Key frames: the carry launch pair next to the input launch and the tracker launch of the same call, and predict_frames with and
without keyframes= (profiles/keyframes.md):

    python tools/bench_keyframes.py [--frames 8] [--samples 20] [--out FILE.json] [--md FILE.md] [--no-model] [--case rgb:20:4]

Frames are 1080p crops of one smoothed-noise texture per channel that move by a random shift of up to 3 pixels per frame (the
whole content moves, so every box is followed: the full cost), RGB and NV12, one stream of `frames` frames per call; every timed
call reads another batch of a ring of more than 300 MB.  The key records hold 20 objects (sides 60 .. 200 pixels) or 300 (sides
20 .. 60) on a grid.

    carry     ops.carry_records (two launches and the scratch allocation) at every = 2, 4, 8, state, out= and records= given;
              `empty`: the same call with key records of count 0 (every walk workgroup leaves at once)
    input     ops.frames_to_input / ops.yuv420_to_input of the same frames (resize_pad_square to 640)
    tracker   ops.track_frames on the carried records of the same call
    end to end  Detector('yolov3_80', synthetic weights).predict_frames(frames, tracker=, input_size=640) without keyframes= and with
              every = 1, 2, 4, 8, the tracker and the KeyFrames reset before every call, alternating call by call

Medians of `samples` after 3 warm-up samples between two device events.  --md writes the tables; what follows the line
`<!-- notes -->` in an existing file is kept."""
import argparse
import json
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from bench_motion import MARGIN, batch, texture, timed  # noqa: E402

NOTES = '<!-- notes -->'
HW = (1080, 1920)


def key_record(objects, lo, hi, shift, rng):
    """An int32 record of `objects` boxes on a grid over the frame, sides in [lo, hi], moved by `shift`."""
    from mydetection_amd import _lib
    cols = int(np.ceil(np.sqrt(objects * 16 / 9)))
    rows = -(-objects // cols)
    k = np.arange(objects)
    cx = (k % cols + 0.5) * HW[1] / cols + shift[0]
    cy = (k // cols + 0.5) * HW[0] / rows + shift[1]
    wh = rng.uniform(lo, hi, (objects, 2))
    rec = np.zeros(_lib.REC_WORDS, np.int32)
    rec[_lib.REC_COUNT] = objects
    rec[_lib.REC_BBOX:_lib.REC_BBOX + 4 * objects] = np.stack([cx, cy, wh[:, 0], wh[:, 1]], axis=1).astype(np.float32).reshape(-1).view(np.int32)
    rec[_lib.REC_SCORE:_lib.REC_SCORE + objects] = np.linspace(0.95, 0.4, objects).astype(np.float32).view(np.int32)
    rec[_lib.REC_CLASS:_lib.REC_CLASS + 2 * objects] = (k % 3).astype(np.int64).view(np.int32)
    return rec


def cell(t):
    return f"{t['median_us']:.1f} ({t['min_us']:.1f} - {t['max_us']:.1f})"


def table(r):
    F = r['frames_per_launch']
    rows = [f'| format | objects | every | carry, {F} frames, us | empty records, us | input launch, us | tracker launch, us | carried / in-between boxes |',
            '|---|---|---|---|---|---|---|---|']
    for c in r['cases']:
        rows.append(f"| {c['format']} | {c['objects']} | {c['every']} | {cell(c['carry'])} | {cell(c['empty'])} | {cell(c['input'])} | {cell(c['tracker'])} | "
                    f"{c['carried']} / {c['between']} |")
    if r.get('end_to_end'):
        rows += ['', f'| predict_frames(tracker=), {F} frames of 1080p, YOLOv3-80 at 640 | us per call | frames per second | objects per frame |', '|---|---|---|---|']
        for e in r['end_to_end']:
            rows.append(f"| {e['name']} | {cell(e['call'])} | {F * 1e6 / e['call']['median_us']:.0f} | {e['objects_per_frame']} |")
    return '\n'.join(rows)


def write_md(path, r):
    notes = ''
    if os.path.exists(path):
        old = open(path).read()
        if NOTES in old:
            notes = old.split(NOTES, 1)[1]
    head = (f"# Key frames: the carry next to the input launch and the tracker launch, and the call end to end (one MI355X)\n\n"
            f"Command: `python tools/bench_keyframes.py` (one stream of {r['frames_per_launch']} frames of 1080p per call, search R = 8, noise textures "
            f"smoothed over 11 pixels that move by up to 3 pixels per frame; the input launch is resize_pad_square to 640; the tracker "
            f"launch runs on the carried records, `max_tracks=512`).  Device `{r['device']}`, shader clock {r['sclk_mhz_at_start']} MHz before "
            f"the first launch and {r['sclk_mhz_at_end']} MHz after the last.  No profiler attached.  A figure is the median of {r['samples']} "
            f"samples after 3 warm-up samples (min - max in brackets), one sample = one call between two device events; every call reads "
            f"another batch of a ring of more than 300 MB, and the launches of a row alternate sample by sample.  `carry` is the whole of "
            f"`ops.carry_records`: two launches and the scratch allocation.  `carried / in-between boxes` counts the boxes the measured "
            f"batches carry against the boxes of their key records times the in-between frames.\n\n")
    with open(path, 'w') as f:
        f.write(head + table(r) + '\n\n' + NOTES + notes)


def clock():
    try:
        return torch.cuda.clock_rate()
    except Exception as e:                                           # the management library is optional
        return f'unavailable ({type(e).__name__})'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=8)
    ap.add_argument('--samples', type=int, default=20)
    ap.add_argument('--out', default=None)
    ap.add_argument('--md', default=None)
    ap.add_argument('--no-model', action='store_true', help='skip the end-to-end part')
    ap.add_argument('--case', default=None, help='FORMAT:OBJECTS:EVERY, e.g. rgb:20:4 -- that row only (for a profiler run of its own)')
    args = ap.parse_args()
    from mydetection_amd import ops, synth
    from mydetection_amd.api import Detector, KeyFrames, Tracker
    from mydetection_amd.models.general import name_to_model
    assert torch.cuda.is_available(), 'bench_keyframes.py measures on the MI355X; there is no CPU path'
    dev = torch.device('cuda', 0)
    F, fmt, (H, W) = args.frames, 'RGB_1_norm', HW
    r = {'device': torch.cuda.get_device_name(0), 'frames_per_launch': F, 'samples': args.samples, 'search': 8, 'cases': [],
         'sclk_mhz_at_start': clock()}
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)
    rng = np.random.Generator(np.random.PCG64(7))
    net = Detector._geometry(types.SimpleNamespace(divisibe=32), H, W, 'resize_pad_square', 640)
    tex = texture(H + MARGIN, W + MARGIN, 11, gen, dev)
    ring = -(-300 * 2 ** 20 // (F * H * W * 3))
    rgb = [batch(tex, HW, F, 3, rng) for _ in range(ring)]
    par = ops.track_params(HW, 'iou')
    for name in ('rgb', 'nv12'):
        if name == 'rgb':
            images, layout = [b for b, _ in rgb], None
        else:
            images = []
            for b, _ in rgb:
                v = b.to(torch.int32)
                y = ((77 * v[..., 0] + 150 * v[..., 1] + 29 * v[..., 2] + 128) >> 8).to(torch.uint8)
                images.append((y, torch.full((F, H // 2, W // 2, 2), 128, dtype=torch.uint8, device=dev)))
            layout = 'nv12'
        for objects, lo, hi in ((20, 60, 200), (300, 20, 60)):
            for every in (2, 4, 8):
                if args.case and args.case != f'{name}:{objects}:{every}':
                    continue
                cset = ops.carry_set(every=every)
                mask = [f % every == 0 for f in range(F)]
                keys = []
                for _, shifts in rgb:                                # the boxes of every key frame sit on the moved content
                    pos = np.cumsum(np.array([s[:2] for s in shifts]), axis=0)
                    krng = np.random.Generator(np.random.PCG64(objects))
                    keys.append(torch.from_numpy(np.stack([key_record(objects, lo, hi, pos[f], krng) for f in range(F) if mask[f]])).to(dev))
                none = torch.zeros_like(keys[0])
                state = ops.carry_state(1, dev)
                first = ops.carry_records(images[0], keys[0], mask, state, cset, layout=layout)
                out, records = {k: first[k] for k in ('how', 'offset', 'sad')}, first['records']
                carried = between = 0
                for img, key in zip(images, keys):                   # what the timed calls compute
                    how = ops.carry_records(img, key, mask, state, cset, layout=layout)['how'][0]
                    carried += int((how == 2).sum())
                    between += objects * (F - sum(mask))
                tstate = ops.track_state(1, 512, dev)
                tout = ops.track_frames(records, tstate, par)
                turn = [0, 0, 0]

                def carry():
                    turn[0] += 1
                    return ops.carry_records(images[turn[0] % ring], keys[turn[0] % ring], mask, state, cset, layout=layout, out=out, records=records)

                def empty():
                    turn[1] += 1
                    return ops.carry_records(images[turn[1] % ring], none, mask, state, cset, layout=layout, out=out, records=records)

                def to_input():
                    turn[2] += 1
                    img = images[turn[2] % ring]
                    return ops.frames_to_input(img, net, fmt) if layout is None else ops.yuv420_to_input(img, layout, net, fmt)
                case = {'format': name, 'objects': objects, 'every': every, 'carried': carried, 'between': between}
                case['carry'], case['empty'], case['input'] = timed([carry, empty, to_input], args.samples)
                ops.carry_records(images[0], keys[0], mask, state, cset, layout=layout, out=out, records=records)
                case['tracker'], = timed([lambda: ops.track_frames(records, tstate, par, out=tout)], args.samples)
                print(json.dumps(case), flush=True)
                r['cases'].append(case)
        del images
    if not args.no_model:
        m, cfg = name_to_model('yolov3_80')
        m.load_state_dict(synth.make_state_dict(m.state_dict()), strict=True)
        det = Detector(model_and_cfg=(m.eval().cuda(), cfg))
        frames = [b for b, _ in rgb]
        variants = [('without keyframes=', None)] + [(f'every = {e}', KeyFrames(every=e)) for e in (1, 2, 4, 8)]
        trackers = [Tracker() for _ in variants]
        turn = [0]
        seen = [0] * len(variants)

        def call(i):
            def fn():
                kf = variants[i][1]
                trackers[i].reset()
                if kf is not None:
                    kf.reset()
                turn[0] += 1
                objs = det.predict_frames(frames[turn[0] % ring], tracker=trackers[i], input_size=640, **({} if kf is None else {'keyframes': kf}))
                seen[i] = round(sum(len(o) for o in objs) / F, 1)
            return fn
        got = timed([call(i) for i in range(len(variants))], args.samples)
        r['end_to_end'] = [{'name': variants[i][0], 'call': got[i], 'objects_per_frame': seen[i]} for i in range(len(variants))]
        for e in r['end_to_end']:
            print(json.dumps(e), flush=True)
    r['sclk_mhz_at_end'] = clock()
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
