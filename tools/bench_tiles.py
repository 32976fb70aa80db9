"""Tiled detection on large frames, piece by piece (profiles/tiles.md):

    python tools/bench_tiles.py [--batch 4] [--height 1080] [--width 1920] [--tile 640] [--input-size 640] [--model yolov3_80]
                                [--samples 20] [--out FILE.json]

The pieces of Detector.predict_frames(frames, tiles=Tiles((tile, tile))) on uint8 frames that are already on the device, each
timed between two device events, `samples` times after a warm-up that also lets the forward batches be graph-captured; medians:

    input     the input launches: one ops.frames_to_input per window over the crop view of all frames
    forward   Detector._records on the input batches (forward + post-process, a hipGraph replay) + records_to_original_
    merge     ops.merge_tile_records on the window records (origins upload, gather launch, post-process launch)
    call      the whole predict_frames call, host work and the final device->host copy of the counts included

and the merge alone for B = 8 frames of T = 7 windows whose records are full (512 detections each, clustered so that the NMS
has work).  Synthetic weights: the times do not depend on the weights, the number of detections does (it is reported)."""
import argparse
import json
import os
import platform
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


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
    return {'median_us': round(statistics.median(out), 1), 'min_us': round(min(out), 1), 'max_us': round(max(out), 1)}


def full_records(B, T, words, dev, seed=1):
    """[T*B, words] records with 512 detections each: 60 clusters per frame, three classes, distinct scores."""
    from mydetection_amd import _lib
    rng = np.random.Generator(np.random.PCG64(seed))
    rec = np.zeros((T, B, words), np.int32)
    for b in range(B):
        ctr, wh, kc = rng.uniform(0, 600, (60, 2)), rng.uniform(20, 120, (60, 2)), rng.integers(0, 3, 60)
        for t in range(T):
            k = rng.integers(0, 60, 512)
            box = np.concatenate([ctr[k] + rng.normal(0, 5, (512, 2)), wh[k] * (1 + rng.normal(0, 0.1, (512, 2)))], 1).astype(np.float32)
            r = rec[t, b]
            r[_lib.REC_COUNT] = 512
            r[_lib.REC_BBOX:_lib.REC_SCORE] = box.view(np.int32).ravel()
            r[_lib.REC_SCORE:_lib.REC_CLASS] = rng.permutation(np.linspace(0.05, 0.95, 512)).astype(np.float32).view(np.int32)
            r[_lib.REC_CLASS:_lib.REC_INDEX] = kc[k].astype(np.int64).view(np.int32)
    return torch.from_numpy(rec.reshape(T * B, words)).to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=4)
    ap.add_argument('--height', type=int, default=1080)
    ap.add_argument('--width', type=int, default=1920)
    ap.add_argument('--tile', type=int, default=640)
    ap.add_argument('--input-size', type=int, default=640)
    ap.add_argument('--model', default='yolov3_80')
    ap.add_argument('--samples', type=int, default=20)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    from mydetection_amd import _lib, ops, synth
    from mydetection_amd.api import Detector, Tiles
    from mydetection_amd.models.general import name_to_model
    assert torch.cuda.is_available(), 'bench_tiles.py measures on the MI355X; there is no CPU path'
    dev = torch.device('cuda', 0)
    m, cfg = name_to_model(args.model)
    m.load_state_dict(synth.make_state_dict(m.state_dict(), args.model), strict=True)
    det = Detector(model_and_cfg=(m.eval().to(dev), cfg))
    B, H, W = args.batch, args.height, args.width
    frames = torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, device=dev, generator=torch.Generator(device=dev).manual_seed(3))
    tiles = Tiles((args.tile, args.tile))
    kw = dict(input_size=args.input_size)
    windows = ops.tile_windows(H, W, tiles.size, tiles.overlap, tiles.full_frame)
    T = len(windows)

    # the pieces, as Detector._records_of_windows strings them together
    by_input = {}
    for i, (_, _, h, w) in enumerate(windows):
        geo = det._geometry(h, w, det.preprocess, args.input_size)
        by_input.setdefault(geo[2], []).append((i, geo))
    xs = {hw: torch.empty((len(ms) * B, 3) + hw, dtype=torch.float32, device=dev) for hw, ms in by_input.items()}

    def build_inputs():
        for hw, members in by_input.items():
            for n, (i, geo) in enumerate(members):
                y0, x0, h, w = windows[i]
                ops.frames_to_input(frames[:, y0:y0 + h, x0:x0 + w], geo, det.model.input_format, out=xs[hw][n * B:(n + 1) * B])

    state = {}

    def forward():
        parts = []
        for hw, members in by_input.items():
            rec = ops.record_views(det._records(xs[hw], det.conf_thres, det.nms_thres)['records'])
            ops.records_to_original_(rec, [geo[3] for _, geo in members for _ in range(B)])
            parts.append(([i for i, _ in members], rec['records']))
        allrec = parts[0][1]
        if len(parts) > 1:
            allrec = allrec.new_empty((T, B, allrec.shape[1]))
            for idx, r in parts:
                allrec[idx] = r.view(len(idx), B, -1)
        state['rec'] = allrec

    origins = [(x0, y0) for y0, x0, _, _ in windows]

    def merge():
        state['merged'] = ops.merge_tile_records(state['rec'], B, T, origins, det.nms_thres)

    def call():
        state['objs'] = det.predict_frames(frames, tiles=tiles, **kw)

    for _ in range(3):                                               # shapes seen, graphs captured
        call()
    build_inputs()
    forward()
    r = {'device': torch.cuda.get_device_name(0), 'host': platform.node(), 'model': args.model, 'frames': [B, H, W],
         'tile': list(tiles.size), 'overlap': tiles.overlap, 'windows': T, 'window_list': [list(w) for w in windows],
         'input_launches': T, 'forward_batches': [[len(ms) * B, 3] + list(hw) for hw, ms in by_input.items()],
         'graphs': [list(k[0]) for k in det._graphs.graphs]}
    try:
        r['sclk_mhz_at_start'] = torch.cuda.clock_rate()
    except Exception as e:                                           # the management library is optional
        r['sclk_mhz_at_start'] = f'unavailable ({type(e).__name__})'
    r['input'] = timed(build_inputs, args.samples)
    r['forward'] = timed(forward, args.samples)
    r['merge'] = timed(merge, args.samples)
    r['call'] = timed(call, args.samples)
    r['window_detections'] = int(ops.record_views(state['rec'].reshape(T * B, -1))['count'].sum())
    r['merged_detections'] = [len(o) for o in state['objs']]
    # the merge alone on full records
    B2, T2 = 8, 7
    rec = full_records(B2, T2, _lib.REC_WORDS, dev)
    org = torch.tensor([(100 * t, 50 * t) for t in range(T2)], dtype=torch.int32, device=dev)
    out = torch.empty((B2, _lib.REC_WORDS), dtype=torch.int32, device=dev)
    for metric in ('iou', 'ios'):
        r[f'merge_full_B8_T7_{metric}'] = timed(lambda: ops.merge_tile_records(rec, B2, T2, org, 0.45, metric, records=out), args.samples)
        r[f'merge_full_B8_T7_{metric}']['kept'] = ops.record_views(out)['count'].tolist()
    try:
        r['sclk_mhz_at_end'] = torch.cuda.clock_rate()
    except Exception as e:
        r['sclk_mhz_at_end'] = f'unavailable ({type(e).__name__})'
    print(json.dumps(r), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(r, f, indent=1)


if __name__ == '__main__':
    main()
