"""Host only: the launch plans of the implicit-GEMM convolutions (mydet_conv_igemm_plan, mydet_conv_b3_plan) of the library in use
(MYDET_LIB_PATH picks another build), written as JSON.  tests/golden/igemm_plans.json is this file as recorded from the commit before
the kernels' shared frame (csrc/igemm_tile.h); tests/test_igemm_plan_host.py replays it.  usage: tools/record_igemm_plans.py OUT.json

What is covered, in the file's own lists (results follow in nested-loop order, outermost first):
  'igemm': shapes x cfgs x cus x ws -- every distinct (B, Ho, Wo, Cin, Cout, taps) of tests/golden/conv_routes.json, the rule's own
           choice (cfg -1) and each tile configuration forced, a whole chip and a quarter of one (the small-grid rule), with and
           without workspace;
  'b3':    b3_shapes x gates x cus x ws -- the rows that hold the 'b3' form, plain and (1x1 rows) gated, default switches;
  'tuned': settings x tuned_shapes x cus x ws -- the shapes of tests/test_b3_plan_host.py under the opt-in forms' switches,
           re-read through mydet_conv_b3_reload_tuning.
A result is [return code, out[0..6]] (out as left by a refused call: zeros).  The file keeps each distinct result once, in 'results', and
the three lists as indices into it; 'b3_shapes' are indices into 'shapes'.  expand() undoes both."""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SWITCHES = ('MYDET_B3_WIDE', 'MYDET_B3_WAVES', 'MYDET_B3_HALF_TILES')
CFGS = [-1, 0, 1, 2, 3, 6, 8, 9]
CUS = [256, 64]
SETTINGS = [[None, None, None], ['1', None, None], [None, '8', None], ['1', None, '0'], [None, '8', '0'], ['1', '8', '0'], ['1', '8', None]]


def tuned_shapes():
    """(M, Cin, Cout, taps) of tests/test_b3_plan_host.py: the GPU cases it pins, its wide-form and eight-wave grids, its boundaries."""
    s = [(32 * 32 * 32, 32, 64, 9), (16 * 1600, 256, 128, 1), (40 * 400, 1024, 512, 1), (16 * 400, 1152, 192, 1), (16 * 1600, 672, 112, 1),
         (8 * 1600, 480, 80, 1), (5 * 33 * 31, 96, 64, 1), (8 * 100, 192, 1152, 1), (40 * 1600, 672, 112, 1)]
    s += [(t * 128, c, 256, 1) for t in (552, 296, 1064, 1320, 640, 641, 64, 65, 16, 648) for c in (1152, 1008, 1024, 512, 496, 4096)]
    s += [(552 * 128, 128, 256, 9), (276 * 128, 1152, 257, 1), (4096, 40, 260, 1), (4096, 40, 193, 1), (4096, 40, 192, 1), (4096, 48, 260, 1),
          (4096, 64, 192, 1), (4096, 64, 193, 1), (4096, 64, 64, 1), (4096, 64, 65, 1), (4096, 64, 1024, 1), (64 * 128, 64, 256, 1),
          (64 * 128 + 1, 64, 256, 1), (128 * 128, 64, 128, 1), (128 * 128 + 1, 64, 128, 1), (150, 64, 136, 9), (150, 768, 136, 1)]
    s += [(t * 128, c, 128, 1) for t in (1, 128, 129, 552, 1064, 1281, 2600) for c in (496, 512, 1008, 1024)]
    return [list(x) for x in s]


def route_shapes():
    rows = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'conv_routes.json')))
    shapes, b3 = set(), set()
    for r in rows:
        k, st, p = r['k'], r['stride'], r['pad']
        Ho, Wo = (r['H'] + p[0] + p[2] - k) // st + 1, (r['W'] + p[1] + p[3] - k) // st + 1
        s = (r['B'], Ho, Wo, r['Cin'], r['Cout'], k * k)
        shapes.add(s)
        if 'b3' in r['forms']:
            b3.add(s)
    return [list(s) for s in sorted(shapes)], [list(s) for s in sorted(b3)]


def call(fn, *args):
    out = (ctypes.c_int32 * 7)()
    rc = fn(*args, out)
    return [rc] + list(out)


def replay(lib, spec):
    """The three result lists of `spec` (its lists of shapes, cfgs, cus, ws, settings) from `lib`."""
    def tune(setting):
        for name, v in zip(SWITCHES, setting):
            os.environ.pop(name, None)
            if v is not None:
                os.environ[name] = v
        lib.mydet_conv_b3_reload_tuning()
    tune([None] * 3)
    res = {'igemm': [], 'b3': [], 'tuned': []}
    try:
        for s in spec['shapes']:
            for cfg in spec['cfgs']:
                for cus in spec['cus']:
                    for ws in spec['ws']:
                        res['igemm'].append(call(lib.mydet_conv_igemm_plan, cfg, *s, ws, cus))
        for s in spec['b3_shapes']:
            for gated in ([0, 1] if s[5] == 1 else [0]):
                for cus in spec['cus']:
                    for ws in spec['ws']:
                        res['b3'].append(call(lib.mydet_conv_b3_plan, *s, gated, ws, cus))
        for setting in spec['settings']:
            tune(setting)
            for M, Cin, Cout, taps in spec['tuned_shapes']:
                for cus in spec['cus']:
                    for ws in spec['ws']:
                        res['tuned'].append(call(lib.mydet_conv_b3_plan, 1, 1, M, Cin, Cout, taps, 0, ws, cus))
    finally:
        tune([None] * 3)
    return res


def expand(rec):
    """A recorded file with its result lists and 'b3_shapes' written out (the form replay() takes and returns)."""
    out = dict(rec, b3_shapes=[rec['shapes'][i] for i in rec['b3_shapes']])
    for key in ('igemm', 'b3', 'tuned'):
        out[key] = [rec['results'][i] for i in rec[key]]
    return out


def main(path):
    from mydetection_amd import _lib, ops
    shapes, b3 = route_shapes()
    spec = {'shapes': shapes, 'cfgs': CFGS, 'cus': CUS, 'ws': [ops.WORKSPACE_BYTES, 0], 'b3_shapes': b3, 'settings': SETTINGS,
            'tuned_shapes': tuned_shapes()}
    got = replay(_lib.lib(), spec)
    results = sorted({tuple(r) for v in got.values() for r in v})
    index = {r: i for i, r in enumerate(results)}
    spec.update(b3_shapes=[shapes.index(s) for s in b3], results=results, **{k: [index[tuple(r)] for r in v] for k, v in got.items()})
    with open(path, 'w') as f:
        f.write('{\n' + ',\n'.join(f' {json.dumps(k)}: {json.dumps(v, separators=(",", ":"))}' for k, v in spec.items()) + '\n}\n')
    print(f"{path}: {len(shapes)} shapes, {' + '.join(str(len(v)) for v in got.values())} plans, {len(results)} distinct, from {_lib.LIB_PATH}")


if __name__ == '__main__':
    main(sys.argv[1])
