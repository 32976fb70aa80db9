"""GPU: two builds of libmydet_hip.so side by side in one process -- the kernels that paint a list of boxes into frames and the chip
sampler (csrc/draw.hip, csrc/redact.hip, csrc/crop.hip; csrc/paint_tile.h) of the parent commit's library (A, --parent-lib;
A' = a second copy of it, --parent-copy) against this tree's (B; --lib names another build to hold against the parent).

    python tools/ab_paint_lib.py --parent-lib OLD.so --parent-copy OLD_COPY.so [--samples 15] [--out FILE.json] [--md FILE.md]
                                 [--part bits|speed|all] [--families draw_rgb,...] [--lib NEW.so]

  bits   every test of tests/test_gpu_draw.py, tests/test_gpu_redact.py and tests/test_gpu_crop.py that needs no detector, each
         parameter set of it, run once through A and once through B on the same seeded inputs: every backing buffer a test checks
         (tests/_paint_targets.py: Target.check) and everything an ops.draw_* / redact_* / crop_* call returns is kept, and the
         two runs are compared buffer by buffer with torch.equal.  A refactor that moves code and reorders no arithmetic differs
         in 0 cases.
  speed  the cases of tools/bench_draw.py (16 frames) and tools/bench_redact.py (8 frames) at 1080 x 1920, RGB and NV12: `reps`
         calls between two device events, alternating A / B / A' sample by sample.  The yardstick of a case is median A; the
         allowance is that case's own |median A - median A'| -- what the measurement cannot resolve.  Per case: the three
         medians; per kernel family (draw / redact x rgb / nv12): their sums.  --families re-measures some families alone.
The libraries are distinct files, so each has its own state.  bind / use are tools/ab_igemm_lib.py's.
"""
import argparse
import inspect
import itertools
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))

import torch                                                          # noqa: E402

from ab_igemm_lib import bind, use                                    # noqa: E402
from mydetection_amd import _lib, ops                                 # noqa: E402

RECORDED_OPS = ('draw_boxes', 'draw_boxes_yuv420', 'draw_records', 'redact_boxes', 'redact_boxes_yuv420', 'redact_records',
                'crop_boxes', 'crop_boxes_yuv420', 'crop_records')


# ---------------------------------------------------------------------------------------------------------------- bits

def kernel_level_cases(module):
    """(name, function, kwargs) for every parameter set of every test of `module` that takes no `detector`."""
    for name, fn in sorted(vars(module).items()):
        if not name.startswith('test_') or not callable(fn) or 'detector' in inspect.signature(fn).parameters:
            continue
        axes = []
        for mark in getattr(fn, 'pytestmark', []):
            if mark.name == 'parametrize':
                names = [n.strip() for n in mark.args[0].split(',')]
                axes.append([dict(zip(names, v if len(names) > 1 else (v,))) for v in mark.args[1]])
        for combo in itertools.product(*axes):
            kwargs = {k: v for d in combo for k, v in d.items()}
            label = ' '.join(f'{k}={v[0] if k == "case" else v}' for k, v in sorted(kwargs.items()))
            yield f'{module.__name__}::{name}[{label}]', fn, kwargs


def part_bits(libs, result):
    import _paint_targets
    import test_gpu_crop
    import test_gpu_draw
    import test_gpu_redact
    kept = []

    def keep(value):
        for t in value if isinstance(value, (tuple, list)) else (value,):
            kept.append(t.detach().clone())

    def recording(fn):
        def wrapped(*args, **kwargs):
            out = fn(*args, **kwargs)
            keep(out)
            return out
        return wrapped

    check = _paint_targets.Target.check
    _paint_targets.Target.check = lambda self, what, skip=None: (keep(self.flat), check(self, what, skip))[1]
    originals = {name: getattr(ops, name) for name in RECORDED_OPS}
    for name, fn in originals.items():
        setattr(ops, name, recording(fn))
    cases, buffers, differ, unrecorded, failed = 0, 0, [], [], []
    try:
        for module in (test_gpu_draw, test_gpu_redact, test_gpu_crop):
            n0 = cases
            for label, fn, kwargs in kernel_level_cases(module):
                got = {}
                for side in ('A', 'B'):
                    use(libs[side])
                    torch.manual_seed(0)
                    kept.clear()
                    try:
                        fn(**kwargs)
                    except AssertionError as e:                     # the test's own check fails in this build: say where, go on
                        failed.append(f'{side} {label}: {str(e)[:200]}')
                        print('FAILED ', failed[-1], flush=True)
                    torch.cuda.synchronize()
                    got[side] = list(kept)
                cases += 1
                buffers += len(got['A'])
                same = len(got['A']) == len(got['B']) and all(a.shape == b.shape and torch.equal(a, b) for a, b in zip(got['A'], got['B']))
                if not same:
                    differ.append(label)
                elif not got['A']:
                    unrecorded.append(label)                        # a test that drives the C entry points itself
                print(('same   ' if same else 'DIFFERS'), len(got['A']), label, flush=True)
            result['bits_' + module.__name__] = cases - n0
    finally:
        _paint_targets.Target.check = check
        for name, fn in originals.items():
            setattr(ops, name, fn)
        kept.clear()
    result['bits_cases'], result['bits_buffers'], result['bits_differ'], result['bits_unrecorded'] = cases, buffers, differ, unrecorded
    result['bits_failed'] = failed
    print(f'bits: {cases} cases, {buffers} buffers, {len(differ)} differ, {len(failed)} failed their own checks', flush=True)


# ---------------------------------------------------------------------------------------------------------------- speed

def speed_cases(dev):
    """(family, label, call) for the cases of tools/bench_draw.py and tools/bench_redact.py."""
    import bench_draw
    import bench_redact
    from mydetection_amd.api import Draw
    H, W = 1080, 1920
    gen = torch.Generator().manual_seed(1)
    frames = torch.randint(0, 256, (16, H, W, 3), dtype=torch.uint8, generator=gen).to(dev)
    y = torch.randint(0, 256, (16, H, W), dtype=torch.uint8, generator=gen).to(dev)
    uv = torch.randint(0, 256, (16, (H + 1) // 2, (W + 1) // 2, 2), dtype=torch.uint8, generator=gen).to(dev)
    for K in (20, 200):
        for rotated in (False, True):
            bd, sd, cd = (torch.from_numpy(a).to(dev) for a in bench_draw.boxes_for(16, K, H, W, rotated, seed=K + rotated))
            for labels in ((), ('class', 'score')):
                st = ops.draw_style(thickness=3, labels=labels, label_height=24)
                what = f'draw {K} boxes{" rotated" if rotated else ""}{" labels" if labels else ""}'
                yield 'draw_rgb', what, lambda bd=bd, sd=sd, cd=cd, st=st: ops.draw_boxes(frames, bd, st, scores=sd, classes=cd)
                yield 'draw_nv12', what, lambda bd=bd, sd=sd, cd=cd, st=st: ops.draw_boxes_yuv420((y, uv), 'nv12', bd, st, scores=sd, classes=cd)
    f8, y8, uv8 = frames[:8], y[:8], uv[:8]
    fill = Draw(fill_alpha=255).style((H, W))
    for K in (8, 32, 256):
        for degrees in (0.0, 30.0):
            bd, sd, cd = (torch.from_numpy(a).to(dev) for a in bench_redact.boxes_for(8, K, H, W, degrees, seed=K + int(degrees)))
            what = f'{K} boxes {degrees:.0f} deg'
            yield 'draw_rgb', f'draw filled {what}', lambda bd=bd, sd=sd, cd=cd: ops.draw_boxes(f8, bd, fill, scores=sd, classes=cd)
            yield 'draw_nv12', f'draw filled {what}', lambda bd=bd, sd=sd, cd=cd: ops.draw_boxes_yuv420((y8, uv8), 'nv12', bd, fill, scores=sd, classes=cd)
            for mode, cells in (('mosaic', (8, 22, 64)), ('smooth', (8, 22, 64)), ('solid', (22,))):
                for cell in cells:
                    st = ops.redact_style(mode, cell)
                    yield 'redact_rgb', f'redact {mode} {cell} {what}', lambda bd=bd, st=st: ops.redact_boxes(f8, bd, st)
                    yield 'redact_nv12', f'redact {mode} {cell} {what}', lambda bd=bd, st=st: ops.redact_boxes_yuv420((y8, uv8), 'nv12', bd, st)


def part_speed(libs, result, samples, reps, families):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    rows, sums = {}, {}
    for family, what, call in speed_cases(torch.device('cuda:0')):
        if families and family not in families:
            continue
        for side in libs:                                           # warm-up: code objects, the redaction workspace
            use(libs[side])
            call()
        torch.cuda.synchronize()
        t = {side: [] for side in libs}
        for _ in range(samples):
            for side in ('A', 'B', 'A2'):
                use(libs[side])
                e0.record()
                for _ in range(reps):
                    call()
                e1.record()
                e1.synchronize()
                t[side].append(e0.elapsed_time(e1) * 1000.0 / reps)
        med = {side: statistics.median(v) for side, v in t.items()}
        key = f'{family}: {what}'
        rows[key] = dict(A=round(med['A'], 2), B=round(med['B'], 2), A2=round(med['A2'], 2), allowance=round(abs(med['A'] - med['A2']), 2),
                         slower_by=round(med['B'] - med['A'], 2))
        tot = sums.setdefault(family, dict(cases=0, A=0.0, B=0.0, A2=0.0))
        tot['cases'] += 1
        for side in ('A', 'B', 'A2'):
            tot[side] += med[side]
        print(key, rows[key], flush=True)
    use(libs['B'])
    result['cases_us'] = rows
    result['families_us'] = {f: {k: (v if k == 'cases' else round(v, 1)) for k, v in tot.items()} for f, tot in sums.items()}
    result['slower_than_allowance'] = {k: v for k, v in rows.items() if v['slower_by'] > v['allowance']}
    print(json.dumps(result['families_us'], indent=1))
    print(f'{len(result["slower_than_allowance"])} of {len(rows)} cases: B slower than A by more than |A - A2|', flush=True)


def markdown(result):
    lines = []
    if 'bits_cases' in result:
        lines += [f'Bits: {result["bits_cases"]} cases, {result["bits_buffers"]} buffers compared, {len(result["bits_differ"])} differ.', '']
    if 'families_us' in result:
        lines += ['| family | cases | A us | B us | A\' us |', '|---|---|---|---|---|']
        lines += [f'| {f} | {v["cases"]} | {v["A"]} | {v["B"]} | {v["A2"]} |' for f, v in result['families_us'].items()]
        lines += ['', '| case | A us | B us | A\' us | allowance | B - A |', '|---|---|---|---|---|---|']
        lines += [f'| {k} | {v["A"]} | {v["B"]} | {v["A2"]} | {v["allowance"]} | {v["slower_by"]} |' for k, v in result['cases_us'].items()]
    return '\n'.join(lines) + '\n'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent-lib', required=True)
    ap.add_argument('--parent-copy', default=None)
    ap.add_argument('--samples', type=int, default=15)
    ap.add_argument('--reps', type=int, default=10, help='calls per timed sample')
    ap.add_argument('--part', default='all', choices=('bits', 'speed', 'all'))
    ap.add_argument('--lib', default=None, help='B: another build instead of this tree\'s')
    ap.add_argument('--families', default=None, help='speed: only these kernel families, comma-separated')
    ap.add_argument('--out', default=None)
    ap.add_argument('--md', default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'this tool needs the MI355X'
    libs = {'A': bind(args.parent_lib), 'B': bind(args.lib) if args.lib else _lib.lib(), 'A2': bind(args.parent_copy or args.parent_lib)}
    result = dict(device=torch.cuda.get_device_name(0), samples=args.samples, reps=args.reps)
    if args.part in ('bits', 'all'):
        part_bits(libs, result)
    use(libs['B'])
    if args.part in ('speed', 'all'):
        part_speed(libs, result, args.samples, args.reps, args.families.split(',') if args.families else None)
    for path, text in ((args.out, json.dumps(result, indent=1)), (args.md, markdown(result))):
        if path:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, 'w') as f:
                f.write(text)
    return 1 if result.get('bits_differ') or result.get('bits_failed') else 0


if __name__ == '__main__':
    sys.exit(main())
