"""Time the post-process kernel's NMS modes (include/mydet.h, "NMS modes") and, next to them, the shipped instances of this
build against the same instances of another build of the library -- the method of profiles/rotnms.md: one process, HIP events
around each launch, the median of 60 launches after 10 warm-up launches, three rounds per function, interleaved (all three
medians are printed: their spread is the run-to-run range).  Results: profiles/nms_modes.md.

    python tools/bench_nms_modes.py [--parent-lib /path/to/libmydet_hip.so] [--json out.json]

Inputs: the worst case of `bench.py --nms-worst` (512 boxes of one image in ONE class; batch 1 and 32; conf 0.005) and the
candidates of one yolov3_80 forward at batch 32, 640^2 (synthetic weights).  Boxes of width 5 get a random angle column.  The
IoS instances run through mydet_merge_tile_records_f32 on the records of a pass that suppresses nothing (T = 1: the gather
launch is inside the span, for both builds).  NMS threshold 0.45.  Every call goes through the C entry points with buffers
allocated once, so a span holds the launch and nothing else."""
import argparse
import contextlib
import ctypes
import io
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mydetection_amd import _lib, ops, synth                              # noqa: E402
from mydetection_amd.models.general import name_to_model                 # noqa: E402

NMS, WARM, ITERS, ROUNDS = 0.45, 10, 60, 3
SHIPPED = ('mydet_postprocess_records_f32', 'mydet_postprocess_records_rot_f32', 'mydet_postprocess_records_rotnms_f32',
           'mydet_merge_tile_records_f32', 'mydet_merge_tile_records_scratch_bytes')


def bind(path):
    h = ctypes.CDLL(path)
    for name in SHIPPED:
        fn = getattr(h, name)
        fn.argtypes = _lib.SIGNATURES[name]
        fn.restype = _lib.c_i64 if name in _lib.RETURNS_I64 else _lib.c_int
    return h


def median_us(call):
    for _ in range(WARM):
        call()
    torch.cuda.synchronize()
    spans = []
    for _ in range(ITERS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        torch.cuda.synchronize()
        spans.append(e0.elapsed_time(e1) * 1e3)
    return float(np.median(spans))


def interleaved(calls):
    """{name: call} -> {name: sorted medians of the three rounds}; a round visits every function once, odd rounds in reverse
    order (so that neither build is always the one measured first)."""
    out = {k: [] for k in calls}
    for r in range(ROUNDS):
        for k in (list(calls) if r % 2 == 0 else reversed(list(calls))):
            out[k].append(round(median_us(calls[k]), 2))
    return {k: sorted(v) for k, v in out.items()}


def worst_case(B, dev):
    rng = np.random.Generator(np.random.PCG64(5 + B))
    cx = rng.random((B, 512), dtype=np.float32) * 600 + 20
    cy = rng.random((B, 512), dtype=np.float32) * 600 + 20
    wh = rng.random((B, 512, 2), dtype=np.float32) * 120 + 20
    bb = torch.from_numpy(np.concatenate([cx[..., None], cy[..., None], wh], axis=-1)).to(dev)
    ci = torch.zeros((B, 512), dtype=torch.int64, device=dev)
    sc = torch.from_numpy((rng.random((B, 512), dtype=np.float32) * 0.9 + 0.05)).to(dev)
    return bb, ci, sc


def model_candidates(dev, batch=32, size=640, config='yolov3_80'):
    with contextlib.redirect_stdout(io.StringIO()):
        model, cfg = name_to_model(config)
    model.load_state_dict(synth.make_state_dict(model.state_dict(), config))
    model = model.eval().to(dev)
    x = (synth.make_images if cfg['general.input_format'] == 'RGB_1' else synth.make_normalized_images)(batch, size, seed=0).to(dev)
    with torch.no_grad():
        bb, ci, sc = model.forward_candidates(x)
    return bb.contiguous(), ci.contiguous(), sc.contiguous()


def bench_input(name, bb, ci, sc, conf, new, parent):
    dev = bb.device
    B, N = sc.shape
    p = ops._ptr
    rng = np.random.Generator(np.random.PCG64(9))
    ang = torch.from_numpy((rng.random((B, N, 1), dtype=np.float32) * 180 - 90)).to(dev)
    bb5 = torch.cat([bb, ang], dim=2).contiguous()
    rec4 = torch.empty((B, _lib.REC_WORDS), dtype=torch.int32, device=dev)
    rec5 = torch.empty((B, _lib.REC_ROT_WORDS), dtype=torch.int32, device=dev)
    scratch = torch.empty((B, N), dtype=torch.int64, device=dev)
    st = ops._stream()
    # tile records for the IoS instances: the selected 512 of every image, nothing suppressed
    tiles4 = ops.postprocess(bb, ci, sc, conf, 1.0)['records'].clone()
    tiles5 = ops.postprocess(bb5, ci, sc, conf, 1.0)['records'].clone()
    org = torch.zeros((1, 2), dtype=torch.int32, device=dev)
    nb4, nb5 = (new.mydet_merge_tile_records_scratch_bytes(B, 1, w) for w in (4, 5))
    ms4, ms5 = (torch.empty(n // 8, dtype=torch.int64, device=dev) for n in (nb4, nb5))

    def shipped(lib):
        return {
            '<4>': lambda: lib.mydet_postprocess_records_f32(p(bb), p(ci), p(sc), B, N, conf, NMS, p(rec4), p(scratch), st),
            '<5>': lambda: lib.mydet_postprocess_records_rot_f32(p(bb5), p(ci), p(sc), B, N, conf, NMS, p(rec5), p(scratch), st),
            '<5, rot>': lambda: lib.mydet_postprocess_records_rotnms_f32(p(bb5), p(ci), p(sc), B, N, conf, NMS, p(rec5), p(scratch), st),
            '<4, ios> (merge, T = 1)': lambda: lib.mydet_merge_tile_records_f32(p(tiles4), 0, _lib.REC_WORDS, B, 1, 4, p(org), NMS, _lib.MERGE_IOS,
                                                                               0, p(rec4), p(ms4), nb4, st),
            '<5, ios> (merge, T = 1)': lambda: lib.mydet_merge_tile_records_f32(p(tiles5), 0, _lib.REC_ROT_WORDS, B, 1, 5, p(org), NMS,
                                                                               _lib.MERGE_IOS, 0, p(rec5), p(ms5), nb5, st),
        }
    calls = {}
    for k, f in shipped(new).items():
        calls['new ' + k] = f
        if parent is not None:
            calls['parent ' + k] = shipped(parent)[k]
    kept = {}
    modes = {}
    for width, b, rec, fn in ((4, bb, rec4, new.mydet_postprocess_records_nms_f32), (5, bb5, rec5, new.mydet_postprocess_records_rot_nms_f32)):
        for kind in ('hard', 'soft-linear', 'soft-gaussian', 'merge'):
            for agn in (False, True):
                if (kind == 'hard' and not agn) or (kind == 'merge' and (width == 5 or not conf > 0)):
                    continue
                mode = ops.nms_mode('bench', ops.Nms(kind, agn), conf, width)
                key = f"{kind}{' agnostic' if agn else ''}, width {width}"
                modes[key] = mode                            # keeps the struct alive
                calls[key] = (lambda fn=fn, b=b, rec=rec, mode=mode:
                              fn(p(b), p(ci), p(sc), B, N, conf, NMS, ctypes.byref(mode), p(rec), p(scratch), st))
    for k, f in calls.items():                               # every call once, checked
        code = f()
        torch.cuda.synchronize()
        assert code == 0, (k, code)
        which = rec5 if k.endswith('width 5') or '<5' in k else rec4
        kept[k] = round(float(which[:, 0].float().mean()), 1)
    times = interleaved(calls)
    passing = float((sc >= conf).sum(dim=1).float().mean())
    return dict(input=name, batch=B, candidates=N, conf=conf, passing_per_image=round(passing, 1), medians_us=times, kept_per_image=kept)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent-lib', default=None, help="another build of libmydet_hip.so (the parent commit's) to time next to this one")
    ap.add_argument('--json', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'needs the MI355X'
    dev = torch.device('cuda:0')
    new = _lib.lib()
    parent = bind(a.parent_lib) if a.parent_lib else None
    results = []
    for B in (1, 32):
        results.append(bench_input(f'nms-worst, one class, 512 boxes, B = {B}', *worst_case(B, dev), 0.005, new, parent))
    results.append(bench_input('yolov3_80 candidates, B = 32, 640^2', *model_candidates(dev), 0.005, new, parent))
    for r in results:
        print(f"## {r['input']}: {r['candidates']} candidates, {r['passing_per_image']} pass conf {r['conf']} per image")
        base = r['medians_us'].get('parent <4>', r['medians_us']['new <4>'])
        for k, v in r['medians_us'].items():
            ratio = '' if k.startswith(('new', 'parent')) else f'  x{v[1] / base[1]:.2f} of the class-aware hard kernel'
            print(f"  {k:40s} {' / '.join(f'{t:.1f}' for t in v)} us   kept {r['kept_per_image'][k]}{ratio}")
    if a.json:
        with open(a.json, 'w') as f:
            json.dump(results, f, indent=1)


if __name__ == '__main__':
    main()
