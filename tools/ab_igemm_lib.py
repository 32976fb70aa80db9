"""GPU: two builds of libmydet_hip.so side by side in one process -- the implicit-GEMM convolutions (csrc/conv_igemm.hip) of the
parent commit's library (A, --parent-lib; A' = a second copy of it, --parent-copy) against this tree's (B).

    python tools/ab_igemm_lib.py --parent-lib OLD.so --parent-copy OLD_COPY.so [--samples 15] [--out FILE.json] [--part bits|speed|all]

  bits   every case of tests/test_gpu_igemm_tiles.py (each tile configuration forced through MYDET_CONV_CFG, and the rule's own) and of
         tests/test_gpu_b3_branches.py (every form x shape x epilogue, the gated ones, the weight split): the outputs of A and B are
         compared with torch.equal.  A refactor that moves code and reorders no arithmetic differs in 0 cases.
  speed  the distinct mydet_conv2d_igemm_f32 / mydet_conv2d_igemm_b3_f32 launches of one eager forward of yolov3_80 (batch 32, 640^2),
         efficientdet-d1 (batch 16) and d1_fcs2_atss (batch 32), recorded here with their full arguments, each timed on synthetic
         operands alternating A / B / A' sample by sample.  The yardstick of a shape is A; the allowance is that shape's own
         |median A - median A'| of the same call -- what the measurement cannot resolve.  Per shape: the three medians; per
         configuration: the medians summed over its launches.
The three libraries are distinct files, so each has its own state (the MYDET_B3_* switches are re-read in all of them).
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import torch                                                          # noqa: E402

from mydetection_amd import _lib, ops, synth                          # noqa: E402
from mydetection_amd.models.general import name_to_model              # noqa: E402

CONFIGS = [('yolov3_80', 32, 640), ('efficientdet-d1', 16, 640), ('d1_fcs2_atss', 32, 640)]
ENTRIES = ('mydet_conv2d_igemm_f32', 'mydet_conv2d_igemm_b3_f32')
SWITCHES = ('MYDET_B3_WIDE', 'MYDET_B3_WAVES', 'MYDET_B3_HALF_TILES')


def bind(path):
    """A library file bound as _lib.lib() binds the package's own."""
    handle = ctypes.CDLL(path)
    for name, argtypes in _lib.SIGNATURES.items():
        fn = getattr(handle, name)
        fn.argtypes = argtypes
        fn.restype = _lib.c_i64 if name in _lib.RETURNS_I64 else _lib.c_int
    assert handle.mydet_abi_version() == _lib.ABI_VERSION, path
    return handle


def use(handle):
    _lib._lib = handle


def retune(libs):
    for h in libs.values():
        h.mydet_conv_b3_reload_tuning()


# ---------------------------------------------------------------------------------------------------------------- bits

def part_bits(libs, result):
    import test_gpu_b3_branches as tb
    import test_gpu_igemm_tiles as tt
    dev = torch.device('cuda:0')
    rows, differ = 0, []

    def both(what, fn):
        nonlocal rows
        out = {}
        for side in ('A', 'B'):
            use(libs[side])
            out[side] = fn()
        torch.cuda.synchronize()
        rows += 1
        if not torch.equal(out['A'], out['B']):
            differ.append(what)
            print('DIFFERS', what, flush=True)

    for name in tt.CASES:
        c = tt._case(name)
        d = tt._device_args(c, dev)
        for cfg in (None,) + tt.IDS:
            os.environ.pop('MYDET_CONV_CFG', None)
            if cfg is not None:
                os.environ['MYDET_CONV_CFG'] = str(cfg)
            both(f'igemm_tiles {name} cfg {cfg}', lambda: tt._run(c, d))
    os.environ.pop('MYDET_CONV_CFG', None)
    result['bits_igemm_tiles'] = rows
    n0 = rows
    for form, f in tb.FORMS.items():
        for k in SWITCHES:
            os.environ.pop(k, None)
        os.environ.update(f['env'])
        retune(libs)
        for shape in tb.PLAIN + tb.KCUT + (tb.GATE if form in tb.GATED_FORMS else ()):
            Cout = tb._cout(shape, form)
            if Cout is None:
                continue
            c = tb._base(shape, Cout)
            use(libs['A'])
            tb._DEVICE.pop(c['name'], None)
            wa = tb._device_args(c, dev)['w3'].clone()
            use(libs['B'])
            tb._DEVICE.pop(c['name'], None)
            d = tb._device_args(c, dev)
            both(f'b3 {form} {c["name"]} weight split', lambda: wa if _lib._lib is libs['A'] else d['w3'])
            for act, residual in (tb.EPILOGUES if shape not in tb.GATE else ((tb.ACT_NONE, False), (tb.ACT_NONE, True))):
                def run():
                    rc, y = tb._b3(c, d, act, residual)
                    assert rc == 0, (form, shape, act, residual, rc)
                    return y
                both(f'b3 {form} {c["name"]} act {act} res {int(residual)}', run)
    for k in SWITCHES:
        os.environ.pop(k, None)
    retune(libs)
    result['bits_b3_branches'] = rows - n0
    result['bits_differ'] = differ
    print(f'bits: {rows} cases ({n0} igemm_tiles, {rows - n0} b3_branches), {len(differ)} differ', flush=True)


# ---------------------------------------------------------------------------------------------------------------- speed

class Recorder:
    """Library proxy: the two entry points' launches of a forward as (entry, scalar arguments, which pointers are null)."""
    def __init__(self, real):
        self._real, self.seq = real, []

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if name not in ENTRIES:
            return fn

        def wrapped(*args):
            code = fn(*args)
            if code == 0:
                self.seq.append((name,) + tuple(a if isinstance(a, int) else bool(a.value) for a in args[:-1]))
            return code
        return wrapped


def launches(lib):
    """{configuration: [launch, ...]} of one eager forward each, through `lib`."""
    out = {}
    for name, B, size in CONFIGS:
        rec = Recorder(lib)
        use(rec)
        m, cfg = name_to_model(name)
        m.load_state_dict(synth.make_state_dict(m.state_dict(), name), strict=True)
        m = m.eval().cuda()
        x = synth.make_image_set(0, B, size, cfg['general.input_format']).cuda()
        with torch.no_grad():
            m.forward_candidates(x) if hasattr(m, 'forward_candidates') else m(x)
        torch.cuda.synchronize()
        out[f'{name}_b{B}_{size}'] = rec.seq
        print(f'{name}_b{B}_{size}: {len(rec.seq)} launches, {len(set(rec.seq))} distinct', flush=True)
        del m, x
        torch.cuda.empty_cache()
    use(lib)
    return out


def operands(launch, lib, ws):
    """Synthetic device operands of a recorded launch -> the argument tuple (without the stream)."""
    entry, x, ldx, w, scale, shift, res, ldr, gate, _, ws_bytes, y, ldy, B, H, W, Cin, Cout, KH, KW, stride, pt, pl, Ho, Wo, act = launch
    g = torch.Generator(device='cuda').manual_seed(1)
    rnd = lambda *s: torch.randn(*s, device='cuda', generator=g)                # noqa: E731
    M, K = B * Ho * Wo, KH * KW * Cin
    t = dict(x=rnd(B * H * W, ldx), w=rnd(Cout, K) / K ** 0.5, scale=rnd(Cout) if scale else None, shift=rnd(Cout) if shift else None,
             res=rnd(M, ldr) if res else None, gate=torch.rand(B, Cin, device='cuda', generator=g) if gate else None,
             y=torch.empty(M, ldy, device='cuda'))
    if entry == 'mydet_conv2d_igemm_b3_f32':
        w3 = torch.empty(lib.mydet_split_bf16_elems(Cout, K), dtype=torch.int16, device='cuda')
        _lib.check(lib.mydet_split_bf16_f32(ops._ptr(t['w']), Cout, K, ops._ptr(w3), ops._stream()), 'mydet_split_bf16_f32')
        t['w'] = w3
    p = ops._ptr
    args = (p(t['x']), ldx, p(t['w']), p(t['scale']), p(t['shift']), p(t['res']), ldr, p(t['gate']), p(ws) if ws_bytes else p(None),
            ws_bytes, p(t['y']), ldy, B, H, W, Cin, Cout, KH, KW, stride, pt, pl, Ho, Wo, act)
    return args, t


def part_speed(libs, result, samples, reps):
    seqs = launches(libs['B'])
    ws = ops.conv_workspace(torch.device('cuda:0'))
    distinct = sorted({l for s in seqs.values() for l in s}, key=str)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    shapes = {}
    for i, launch in enumerate(distinct):
        args, keep = operands(launch, libs['B'], ws)
        stream = ops._stream()
        fns = {side: getattr(h, launch[0]) for side, h in libs.items()}
        for fn in fns.values():                                     # warm-up: attributes, caches
            _lib.check(fn(*args, stream), launch[0])
        torch.cuda.synchronize()
        t = {side: [] for side in fns}
        for _ in range(samples):
            for side in ('A', 'B', 'A2'):
                e0.record()
                for _ in range(reps):
                    fns[side](*args, stream)
                e1.record()
                e1.synchronize()
                t[side].append(e0.elapsed_time(e1) * 1000.0 / reps)
        med = {side: statistics.median(v) for side, v in t.items()}
        key = launch[0].replace('mydet_conv2d_', '') + ' ' + ' '.join(str(int(a)) for a in launch[1:])
        shapes[key] = dict(A=round(med['A'], 3), B=round(med['B'], 3), A2=round(med['A2'], 3),
                           allowance=round(abs(med['A'] - med['A2']), 3), slower_by=round(med['B'] - med['A'], 3))
        del keep
        if i % 20 == 0:
            print(f'speed {i + 1}/{len(distinct)} {key}: {shapes[key]}', flush=True)
    result['shapes_us'] = shapes
    result['argument_order'] = ('entry, then null flags / scalars of: x ldx w scale shift residual ldr gate workspace workspace_bytes y ldy '
                                'B H W Cin Cout KH KW stride pad_t pad_l Ho Wo act')
    result['configs_us'] = {}
    for cfg, seq in seqs.items():
        tot = {side: 0.0 for side in ('A', 'B', 'A2')}
        for launch in seq:
            key = launch[0].replace('mydet_conv2d_', '') + ' ' + ' '.join(str(int(a)) for a in launch[1:])
            for side in tot:
                tot[side] += shapes[key][side]
        result['configs_us'][cfg] = dict(launches=len(seq), distinct=len(set(seq)), **{s: round(v, 1) for s, v in tot.items()})
    over = {k: v for k, v in shapes.items() if v['slower_by'] > v['allowance']}
    result['slower_than_allowance'] = over
    print(json.dumps(result['configs_us'], indent=1))
    print(f'{len(over)} of {len(shapes)} shapes: B slower than A by more than |A - A2|', flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent-lib', required=True)
    ap.add_argument('--parent-copy', default=None)
    ap.add_argument('--samples', type=int, default=15)
    ap.add_argument('--reps', type=int, default=4, help='launches per timed sample')
    ap.add_argument('--part', default='all', choices=('bits', 'speed', 'all'))
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'this tool needs the MI355X'
    libs = {'A': bind(args.parent_lib), 'B': _lib.lib(), 'A2': bind(args.parent_copy or args.parent_lib)}
    result = dict(device=torch.cuda.get_device_name(0), samples=args.samples, reps=args.reps)
    if args.part in ('bits', 'all'):
        part_bits(libs, result)
    use(libs['B'])
    if args.part in ('speed', 'all'):
        part_speed(libs, result, args.samples, args.reps)
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(result, f, indent=1)
    return 1 if result.get('bits_differ') else 0


if __name__ == '__main__':
    sys.exit(main())
