"""Appearance: what the descriptor launch and the tracker launch with an appearance cost, next to the launches they stand beside,
and the existing tracker entry points against another build of the library (profiles/appearance.md):

    python tools/bench_appearance.py [--frames 8] [--samples 30] [--parent-lib OLD/libmydet_hip.so] [--out FILE.json] [--md FILE.md]

One stream of `frames` 1080p frames per call, 20 and 300 objects per frame (the records of tools/bench_track.py, rotated boxes,
`max_tracks=512`); the frames are uniform noise in blocks of 8 x 8 pixels, so the descriptors of different objects differ.

    descriptor   ops.appear_records on RGB frames and on NV12 planes, out= given, next to ops.crop_records of the same records
                 (128 x 64 uint8 chips, dst= given) in the same run
    tracker      ops.track_frames with appear= (gate 0.3, reid 0.6; the descriptors of the frames) next to the same call without
                 it (mydet_track_frames_f32) on the same records in the same run
    parent       with --parent-lib: mydet_track_frames_f32, _assoc_f32 (score bands) and _motion_f32 of that library and of this
                 one on the same records through the same ctypes call, the parent library timed TWICE in the same alternation:
                 the difference of its two medians is the run-to-run spread the comparison is read against

Medians of `samples` after 3 warm-up samples between two device events, the launches of a row alternating sample by sample.
--md writes the tables; what follows the line `<!-- notes -->` in an existing file is kept."""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from bench_motion import NOTES, timed  # noqa: E402
from bench_track import records  # noqa: E402

HW = (1080, 1920)
CHIP = (128, 64)
ENTRIES = ('mydet_track_frames_f32', 'mydet_track_frames_assoc_f32', 'mydet_track_frames_motion_f32')


def noise_frames(F, gen, dev):
    coarse = torch.randint(0, 256, (F, HW[0] // 8, HW[1] // 8, 3), generator=gen, device=dev, dtype=torch.uint8)
    return coarse.repeat_interleave(8, dim=1).repeat_interleave(8, dim=2).contiguous()


def nv12_of(rgb):
    v = rgb.to(torch.int32)
    y = ((77 * v[..., 0] + 150 * v[..., 1] + 29 * v[..., 2] + 128) >> 8).to(torch.uint8)
    uv = torch.stack([((-43 * v[..., 0] - 85 * v[..., 1] + 128 * v[..., 2] + 128) >> 8) + 128,
                      ((128 * v[..., 0] - 107 * v[..., 1] - 21 * v[..., 2] + 128) >> 8) + 128], dim=-1).clamp(0, 255).to(torch.uint8)
    return y.contiguous(), uv[:, ::2, ::2].contiguous()


def bind(path):
    """Another build of the library, bound with this package's signatures (the entry points timed here did not change)."""
    from mydetection_amd import _lib
    handle = ctypes.CDLL(path)
    for name in ENTRIES + ('mydet_track_reset',):
        fn = getattr(handle, name)
        fn.argtypes, fn.restype = _lib.SIGNATURES[name], ctypes.c_int
    return handle


def raw_call(handle, entry, rec, state, par, out, assoc, shift, F):
    """One of the three existing entry points of `handle` through ctypes, as ops.track_frames calls it."""
    args = (rec.data_ptr(), rec.stride(0) * F, rec.stride(0), 1, F, 5, ctypes.byref(par), 512, state.data_ptr(), out['box'].data_ptr(),
            out['score'].data_ptr(), out['cls'].data_ptr(), out['id'].data_ptr(), out['missed'].data_ptr(), out['count'].data_ptr(),
            out['dropped'].data_ptr())
    stream = torch.cuda.current_stream().cuda_stream
    if entry == ENTRIES[0]:
        code = getattr(handle, entry)(*args, stream)
    elif entry == ENTRIES[1]:
        code = getattr(handle, entry)(*args, ctypes.byref(assoc), stream)
    else:
        code = getattr(handle, entry)(*args, ctypes.byref(assoc), shift.data_ptr(), stream)
    assert code == 0, (entry, code)


def cell(t):
    return f"{t['median_us']:.1f} ({t['min_us']:.1f} - {t['max_us']:.1f})"


def tables(r):
    F = r['frames_per_launch']
    rows = [f'| objects | descriptor RGB, {F} frames, us | descriptor NV12, us | crop RGB (128 x 64 chips), us | crop NV12, us |', '|---|---|---|---|---|']
    for c in r['descriptor']:
        rows.append(f"| {c['objects']} | {cell(c['appear_rgb'])} | {cell(c['appear_nv12'])} | {cell(c['crop_rgb'])} | {cell(c['crop_nv12'])} |")
    rows += ['', f'| objects | tracker with appearance, {F} frames, us | mydet_track_frames_f32, us | ratio | re-identified / gated in the last call |',
             '|---|---|---|---|---|']
    for c in r['tracker']:
        rows.append(f"| {c['objects']} | {cell(c['appear'])} | {cell(c['plain'])} | {c['appear']['median_us'] / c['plain']['median_us']:.2f} | "
                    f"{c['reidentified']} / {c['matched']} matched |")
    if r.get('parent'):
        rows += ['', '| objects | entry point | parent, first, us | this build, us | parent, second, us | this - parent (mean of both), us | parent spread, us |',
                 '|---|---|---|---|---|---|---|']
        for c in r['parent']:
            a, n, b = c['parent_a']['median_us'], c['new']['median_us'], c['parent_b']['median_us']
            rows.append(f"| {c['objects']} | `{c['entry']}` | {cell(c['parent_a'])} | {cell(c['new'])} | {cell(c['parent_b'])} | {n - (a + b) / 2:+.1f} | {abs(a - b):.1f} |")
    return '\n'.join(rows)


def write_md(path, r):
    notes = ''
    if os.path.exists(path):
        old = open(path).read()
        if NOTES in old:
            notes = old.split(NOTES, 1)[1]
    head = (f"# Appearance: the descriptor launch and the tracker launch with an appearance (one MI355X)\n\n"
            f"Command: `python tools/bench_appearance.py` (one stream of {r['frames_per_launch']} frames of {HW[0]} x {HW[1]} per call; the records of "
            f"`tools/bench_track.py`, rotated boxes, `max_tracks=512`; noise frames in 8 x 8 blocks).  Device `{r['device']}`, shader clock "
            f"{r['sclk_mhz_at_start']} MHz before the first launch and {r['sclk_mhz_at_end']} MHz after the last.  No profiler attached.  A figure is the "
            f"median of {r['samples']} samples after 3 warm-up samples (min - max in brackets), one sample = one call between two device events, every "
            f"buffer on the device and `out=` / `dst=` given; the launches of a row alternate sample by sample.\n\n")
    with open(path, 'w') as f:
        f.write(head + tables(r) + '\n\n' + NOTES + notes)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=8)
    ap.add_argument('--samples', type=int, default=30)
    ap.add_argument('--parent-lib', default=None)
    ap.add_argument('--out', default=None)
    ap.add_argument('--md', default=None)
    args = ap.parse_args()
    from mydetection_amd import _lib, ops
    assert torch.cuda.is_available(), 'bench_appearance.py measures on the MI355X; there is no CPU path'
    dev = torch.device('cuda', 0)
    F = args.frames
    r = {'device': torch.cuda.get_device_name(0), 'frames_per_launch': F, 'samples': args.samples, 'descriptor': [], 'tracker': [], 'parent': []}

    def clock():
        try:
            return torch.cuda.clock_rate()
        except Exception as e:                                       # the management library is optional
            return f'unavailable ({type(e).__name__})'
    r['sclk_mhz_at_start'] = clock()
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)
    ring = [noise_frames(F, gen, dev) for _ in range(4)]
    planes = [nv12_of(b) for b in ring]
    par = ops.track_params(HW, 'rotated')
    parent = bind(args.parent_lib) if args.parent_lib else None
    for objects in (20, 300):
        rec = torch.from_numpy(records(1, F, objects, 5, seed=objects + 1)).to(dev)
        views = ops.record_views(rec)
        desc = ops.appear_records(ring[0], views)
        chips = ops.crop_records(ring[0], views, CHIP)
        turn = [0]

        def nxt():
            turn[0] += 1
            return turn[0] % len(ring)
        c = {'objects': objects, 'samples_per_box': 512}
        c['appear_rgb'], c['crop_rgb'], c['appear_nv12'], c['crop_nv12'] = timed(
            [lambda: ops.appear_records(ring[nxt()], views, out=desc), lambda: ops.crop_records(ring[nxt()], views, CHIP, dst=chips),
             lambda: ops.appear_records(planes[nxt()], views, layout='nv12', out=desc),
             lambda: ops.crop_records(planes[nxt()], views, CHIP, layout='nv12', dst=chips)], args.samples)
        print(json.dumps(c), flush=True)
        r['descriptor'].append(c)

        desc = ops.appear_records(ring[0], views)
        tstate, astate, pstate = ops.track_state(1, 512, dev), ops.appear_state(1, 512, dev), ops.track_state(1, 512, dev)
        aset = ops.appear_set(0.3, 0.6, 0.9, 2.0, 0.3)
        aout = ops.track_frames(rec, tstate, par, appear=(aset, desc, astate))
        pout = ops.track_frames(rec, pstate, par)
        t = {'objects': objects}
        t['appear'], t['plain'] = timed([lambda: ops.track_frames(rec, tstate, par, out=aout, appear=(aset, desc, astate)),
                                         lambda: ops.track_frames(rec, pstate, par, out=pout)], args.samples)
        t['live_tracks'] = aout['count'][:, -1].tolist()
        t['reidentified'], t['matched'] = int((aout['how'] == 3).sum()), int(((aout['how'] >= 1) & (aout['how'] <= 3)).sum())
        print(json.dumps(t), flush=True)
        r['tracker'].append(t)

        if parent is not None:
            bands = ops.track_assoc('greedy', 0.2, 0.5, 0.3)
            shift = torch.zeros((1, F, 4), dtype=torch.int32, device=dev)
            shift[..., 2] = 1
            for entry in ENTRIES:
                assoc = bands if entry != ENTRIES[0] else None
                states = [ops.track_state(1, 512, dev) for _ in range(3)]
                outs = [{k: torch.empty_like(v) for k, v in pout.items()} for _ in range(3)]
                libs = (parent, _lib.lib(), parent)
                fns = [(lambda h=h, s=s, o=o: raw_call(h, entry, rec, s, par, o, assoc, shift, F)) for h, s, o in zip(libs, states, outs)]
                p = {'objects': objects, 'entry': entry}
                p['parent_a'], p['new'], p['parent_b'] = timed(fns, args.samples)
                torch.cuda.synchronize()
                p['same_bits'] = bool(all(torch.equal(outs[0][k], outs[1][k]) for k in outs[0]) and torch.equal(states[0], states[1]))
                print(json.dumps(p), flush=True)
                r['parent'].append(p)
    r['sclk_mhz_at_end'] = clock()
    print(tables(r), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(r, f, indent=1)
    if args.md:
        os.makedirs(os.path.dirname(os.path.abspath(args.md)), exist_ok=True)
        write_md(args.md, r)


if __name__ == '__main__':
    main()
