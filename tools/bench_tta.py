"""Test-time augmentation, piece by piece (profiles/tta.md):

    python tools/bench_tta.py [--batch 4] [--height 1080] [--width 1920] [--input-size 640] [--model yolov3_80] [--samples 20]
                              [--out FILE.json]

Each piece is timed between two device events, `samples` times after a warm-up that also lets the forward batches be
graph-captured; medians:

    input      ops.frames_to_input on the uint8 frames (already on the device), flip = 0, 1, 2, 3: the mirrored launch against
               the unmirrored one, and against what a user did before -- torch.flip (a copy) + the unmirrored launch
    fuse       ops.fuse_view_records (flips in the kernel arguments, gather launch, then the post-process kernel or the WBF
               kernel), `records=` given, for V = 2, 3 and 8 views of B frames:
                 step    the records of a YOLOv3-80 step on the frames and their mirrored copies (what the detector found)
                 full    512 detections per view in 60 clusters of three classes: the top-512 cut and the NMS both have work
                 chain   the worst case of WBF: V x 512 candidates of ONE class on separate cells, every view the same boxes --
                         one dependent chain of V*512 steps against 512 clusters
    call       predict_frames(frames, augment=Augment(...)) end to end, host work and the device->host copy of the counts
               included, against the call without augment and against the baseline a user had before: torch.flip copies, one
               predict_frames call per view, the coordinates negated on the host, ops.merge_tile_records with zero origins

Synthetic weights: the times do not depend on the weights, the number of detections does (it is reported)."""
import argparse
import json
import os
import platform
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FLIP_DIMS = {1: [2], 2: [1], 3: [1, 2]}


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


def pack(rec, box, score, cls):
    from mydetection_amd import _lib
    n = len(box)
    rec[_lib.REC_COUNT] = n
    rec[_lib.REC_BBOX:_lib.REC_BBOX + 4 * n] = np.ascontiguousarray(box, np.float32).view(np.int32).ravel()
    rec[_lib.REC_SCORE:_lib.REC_SCORE + n] = np.asarray(score, np.float32).view(np.int32)
    rec[_lib.REC_CLASS:_lib.REC_CLASS + 2 * n] = np.asarray(cls, np.int64).view(np.int32)


def full_records(B, V, dev, seed=1):
    """[V*B, words] records with 512 detections each: 60 clusters per frame, three classes, distinct scores."""
    from mydetection_amd import _lib
    rng = np.random.Generator(np.random.PCG64(seed))
    rec = np.zeros((V, B, _lib.REC_WORDS), np.int32)
    for b in range(B):
        ctr, wh, kc = rng.uniform(0, 600, (60, 2)), rng.uniform(20, 120, (60, 2)), rng.integers(0, 3, 60)
        for v in range(V):
            k = rng.integers(0, 60, 512)
            box = np.concatenate([ctr[k] + rng.normal(0, 5, (512, 2)), wh[k] * (1 + rng.normal(0, 0.1, (512, 2)))], 1)
            pack(rec[v, b], box, rng.permutation(np.linspace(0.05, 0.95, 512)), kc[k])
    return torch.from_numpy(rec.reshape(V * B, -1)).to(dev)


def chain_records(B, V, dev, seed=2):
    """[V*B, words]: every view holds the same 512 boxes of one class on separate cells, scores distinct over all views.  WBF
    founds 512 clusters and then joins (V - 1) * 512 candidates to them, each against all 512 clusters: the longest chain."""
    from mydetection_amd import _lib
    rng = np.random.Generator(np.random.PCG64(seed))
    rec = np.zeros((V, B, _lib.REC_WORDS), np.int32)
    cell = np.arange(512)
    box = np.stack([5 + 10 * (cell % 32), 5 + 10 * (cell // 32), np.full(512, 8), np.full(512, 8)], 1)
    for b in range(B):
        scores = rng.permutation(np.linspace(0.05, 0.95, V * 512)).reshape(V, 512)
        for v in range(V):
            pack(rec[v, b], box + rng.normal(0, 0.2, (512, 4)), scores[v], np.zeros(512))
    return torch.from_numpy(rec.reshape(V * B, -1)).to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=4)
    ap.add_argument('--height', type=int, default=1080)
    ap.add_argument('--width', type=int, default=1920)
    ap.add_argument('--input-size', type=int, default=640)
    ap.add_argument('--model', default='yolov3_80')
    ap.add_argument('--samples', type=int, default=20)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    from mydetection_amd import _lib, ops, synth
    from mydetection_amd.api import Augment, Detector
    from mydetection_amd.models.general import name_to_model
    assert torch.cuda.is_available(), 'bench_tta.py measures on the MI355X; there is no CPU path'
    dev = torch.device('cuda', 0)
    m, cfg = name_to_model(args.model)
    m.load_state_dict(synth.make_state_dict(m.state_dict(), args.model), strict=True)
    det = Detector(model_and_cfg=(m.eval().to(dev), cfg))
    B, H, W = args.batch, args.height, args.width
    frames = torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, device=dev, generator=torch.Generator(device=dev).manual_seed(3))
    kw = dict(input_size=args.input_size)
    geo = det._geometry(H, W, det.preprocess, args.input_size)
    r = {'device': torch.cuda.get_device_name(0), 'host': platform.node(), 'model': args.model, 'frames': [B, H, W],
         'input': [B, 3] + list(geo[2]), 'samples': args.samples}
    try:
        r['sclk_mhz_at_start'] = torch.cuda.clock_rate()
    except Exception as e:                                           # the management library is optional
        r['sclk_mhz_at_start'] = f'unavailable ({type(e).__name__})'

    # 1. the input launch
    x = torch.empty((B, 3) + tuple(geo[2]), dtype=torch.float32, device=dev)
    for flip in (0, 1, 2, 3):
        r[f'input_flip{flip}'] = timed(lambda: ops.frames_to_input(frames, geo, det.model.input_format, out=x, flip=flip), args.samples)
        if flip:
            r[f'input_copy_flip{flip}'] = timed(lambda: ops.frames_to_input(torch.flip(frames, FLIP_DIMS[flip]), geo, det.model.input_format,
                                                                            out=x), args.samples)

    # 2. the fusion launch pair
    plans = {2: [0, 1], 3: [0, 1, 2], 8: [0, 1, 2, 3, 0, 1, 2, 3]}
    out = torch.empty((B, _lib.REC_WORDS), dtype=torch.int32, device=dev)
    for V, flips in plans.items():
        mirrored = torch.cat([torch.flip(frames, FLIP_DIMS[f]) if f else frames for f in flips[:4]])
        objs = det.predict_frames(mirrored, **kw)
        nv = min(V, 4)
        step = np.zeros((V, B, _lib.REC_WORDS), np.int32)
        for v in range(V):
            for b in range(B):
                o = objs[(v % nv) * B + b]
                pack(step[v, b], o.bboxes.cpu().numpy()[:, :4], o.scores.cpu().numpy(), o.cats.cpu().numpy())
        sets = {'step': torch.from_numpy(step.reshape(V * B, -1)).to(dev), 'full': full_records(B, V, dev), 'chain': chain_records(B, V, dev)}
        for name, rec in sets.items():
            for kind in ('nms', 'wbf'):
                key = f'fuse_{name}_V{V}_{kind}'
                r[key] = timed(lambda: ops.fuse_view_records(rec, B, V, flips, (H, W), 0.45, kind, records=out), args.samples)
                r[key]['candidates'] = int(ops.record_views(rec)['count'].view(V, B).sum(0).max())
                r[key]['kept'] = ops.record_views(out)['count'].tolist()

    # 3. the call, against the baseline of the parent commit
    def baseline(flips):
        recs = []
        for f in flips:
            objs = det.predict_frames(torch.flip(frames, FLIP_DIMS[f]) if f else frames, **kw)
            view = np.zeros((B, _lib.REC_WORDS), np.int32)
            for b, o in enumerate(objs):
                box = o.bboxes.cpu().numpy()[:, :4].copy()
                if f & 1:
                    box[:, 0] = np.float32(W) - box[:, 0]
                if f & 2:
                    box[:, 1] = np.float32(H) - box[:, 1]
                pack(view[b], box, o.scores.cpu().numpy(), o.cats.cpu().numpy())
            recs.append(view)
        rec = torch.from_numpy(np.stack(recs).reshape(len(flips) * B, -1)).to(dev)
        return ops.merge_tile_records(rec, B, len(flips), [(0, 0)] * len(flips), det.nms_thres)

    state = {}
    calls = {'plain': (lambda: det.predict_frames(frames, **kw)),
             'augment_h': (lambda: det.predict_frames(frames, augment=Augment(hflip=True), **kw)),
             'baseline_h': (lambda: baseline([0, 1])),
             'augment_hv4': (lambda: det.predict_frames(frames, augment=Augment(hflip=True, vflip=True), **kw)),
             'baseline_hv4': (lambda: baseline([0, 1, 2, 3])),
             'augment_h_wbf': (lambda: det.predict_frames(frames, augment=Augment(hflip=True, fuse='wbf'), **kw)),
             'augment_yolov5': (lambda: det.predict_frames(frames, augment=Augment(views=((1.0, ''), (0.83, 'h'), (0.67, ''))), **kw))}
    for name, fn in calls.items():
        for _ in range(3):                                           # shapes seen, graphs captured
            state[name] = fn()
        r[f'call_{name}'] = timed(fn, args.samples)
    r['detections'] = {name: ([len(o) for o in v] if isinstance(v, list) else v['count'].tolist()) for name, v in state.items()}
    r['graphs'] = [list(k[0]) for k in det._graphs.graphs]
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
