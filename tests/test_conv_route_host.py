"""CPU-only checks of the conv routing (ops.conv_route, ops.conv_forms, the launch loop of ops.conv2d over ops.CONV_LAUNCHERS).

tests/golden/conv_routes.json holds one row per distinct ops.conv2d call of an eager forward of the shipped configurations (yolov3_80,
efficientdet-d1, d1_fcs2_atss at their benchmark batches and at half of them -- a graph lane --, ulo5m, rapid, d1_rapid, d1_fcs2s at their
fixture sizes), recorded on the MI355X before the routes were tabulated: the layer, the forms its caller held, the entry points that
refused (none did) and the one that ran."""
import ctypes
import json
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAY_REFUSE = ('conv_p3', 'conv_igemm_b3')
UNSUPP = -2


def _rows():
    with open(os.path.join(ROOT, 'tests', 'golden', 'conv_routes.json')) as f:
        return json.load(f)


def _route(ops, r):
    return ops.conv_route(r['B'], r['H'], r['W'], r['Cin'], r['Cout'], r['k'], r['stride'], tuple(r['pad']), r['act'], gated=r['gated'],
                          ldy=r['ldy'], ldr=r['ldr'], forms=set(r['forms']), b3_min_rows=r['b3_min_rows'])


def test_recorded_layers_keep_their_route():
    """Every recorded layer: the route starts with the launchers that answered -- the refused ones, then the one that ran; every element
    before the last is a launcher that may refuse, the last one is not, and each is a row of the launcher table."""
    from mydetection_amd import ops
    rows = _rows()
    assert len(rows) > 300 and {r['family'] for r in rows} == set(ops.CONV_LAUNCHERS)
    for r in rows:
        route = _route(ops, r)
        answered = tuple(r['refused']) + (r['family'],)
        assert route[:len(answered)] == answered, (r, route)
        assert all(f in MAY_REFUSE for f in route[:-1]) and route[-1] not in MAY_REFUSE and len(set(route)) == len(route), (r, route)
        assert set(route) <= set(ops.CONV_LAUNCHERS)


def test_recorded_forms_are_worth_preparing():
    """Every form a recorded caller held is one conv_forms names for the layer (the callers prepare what it names, no more), and every
    launcher of a route reads the OHWI weight or a form the caller held."""
    from mydetection_amd import ops
    for r in _rows():
        among = ops.CONV_FORMS if 'wino' in r['forms'] or 'wino4' in r['forms'] else frozenset(r['forms'])
        assert set(r['forms']) <= ops.conv_forms(r['Cout'], r['Cin'], r['k'], r['stride'], tuple(r['pad']), r['gated'], r['act'], among=among), r
        assert all(ops.CONV_LAUNCHERS[f][2] in (None, *r['forms']) for f in _route(ops, r)), r


def test_conv_forms_rules(monkeypatch):
    from mydetection_amd import ops
    pad1, pad0 = (1, 1, 1, 1), (0, 0, 0, 0)
    leaky, none, swish = ops.ACT_LEAKY, ops.ACT_NONE, ops.ACT_SWISH
    for name in ('WINOGRAD', 'WINOGRAD4', 'SPLIT_BF16'):
        monkeypatch.setattr(ops, name, True)
    assert ops.conv_forms(64, 32, 3, 1, pad1, False, leaky) == {'wino', 'b3'}              # below F(4x4)'s channels: conv_p3 may come first
    assert ops.conv_forms(128, 64, 3, 1, pad1, False, leaky) == {'wino', 'wino4'}          # a Winograd form takes it at every size
    assert ops.conv_forms(128, 64, 3, 2, pad1, False, leaky) == {'b3'}
    assert ops.conv_forms(128, 64, 3, 1, pad0, False, leaky) == {'b3'}
    assert ops.conv_forms(81, 88, 3, 1, pad1, False, none) == set()                          # Cout % 4: no transform; Cin % 16: no planes
    assert ops.conv_forms(84, 88, 3, 1, pad1, False, none) == {'wino', 'wino4'}
    assert ops.conv_forms(84, 36, 3, 1, pad1, False, none) == set()                          # Cin % 8, below WINO4_MIN_CIN, Cin % 16
    assert ops.conv_forms(255, 1024, 1, 1, pad0, False, none) == {'b3'}
    assert ops.conv_forms(96, 24, 1, 1, pad0, False, swish) == {'b3'}                        # 1x1: Cin % 4, the last slab zero-filled
    assert ops.conv_forms(96, 24, 3, 2, pad1, False, leaky) == set()
    assert ops.conv_forms(40, 240, 1, 1, pad0, True, none) == {'b3'}                         # gated: 1x1 without activation only
    assert ops.conv_forms(40, 240, 1, 1, pad0, True, swish) == set()
    assert ops.conv_forms(128, 64, 3, 1, pad1, False, leaky, among={'b3'}) == {'b3'}       # a caller that holds no Winograd form
    assert ops.conv_forms(64, 32, 3, 1, pad1, False, leaky, among={'wino', 'wino4'}) == {'wino'}
    monkeypatch.setattr(ops, 'WINOGRAD4', False)
    assert ops.conv_forms(128, 64, 3, 1, pad1, False, leaky) == {'wino'}
    monkeypatch.setattr(ops, 'WINOGRAD', False)
    assert ops.conv_forms(128, 64, 3, 1, pad1, False, leaky) == {'b3'}
    monkeypatch.setattr(ops, 'SPLIT_BF16', False)
    assert ops.conv_forms(128, 64, 3, 1, pad1, False, leaky) == set()


# (x, ldx, weight, scale, shift, residual, ldr, out, ldy, B, H, W, Cin, Cout, act) among each entry point's arguments (include/mydet.h)
ENTRY_ARGS = {
    'mydet_conv3x3_p3_f32': (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 15),
    'mydet_conv2d_wino4_f32': (0, 1, 2, 3, 4, 5, 6, 9, 10, 11, 12, 13, 14, 15, 16),
    'mydet_conv2d_wino_f32': (0, 1, 2, 3, 4, 5, 6, 9, 10, 11, 12, 13, 14, 15, 16),
    'mydet_conv2d_igemm_b3_f32': (0, 1, 2, 3, 4, 5, 6, 10, 11, 12, 13, 14, 15, 16, 24),
    'mydet_conv2d_igemm_f32': (0, 1, 2, 3, 4, 5, 6, 10, 11, 12, 13, 14, 15, 16, 24),
}
ARG_NAMES = ('x', 'ldx', 'weight', 'scale', 'shift', 'residual', 'ldr', 'out', 'ldy', 'B', 'H', 'W', 'Cin', 'Cout', 'act')


class StandInLibrary:
    """Stands in for _lib.lib(): the host-side plan and size functions are the built library's own; a conv entry point is recorded with
    its arguments (pointers as integers) and answers the code chosen for it (default 0) without launching anything."""
    def __init__(self, real, codes=None):
        self.real, self.codes, self.calls = real, dict(codes or {}), []

    def __getattr__(self, name):
        if name not in ENTRY_ARGS:
            assert 'plan' in name or name.endswith(('_bytes', '_floats', '_elems')), f'{name} is no host-side function'
            return getattr(self.real, name)

        def entry(*args):
            values = [a if isinstance(a, int) else a.value for a in args]
            self.calls.append((name, dict(zip(ARG_NAMES, (values[i] for i in ENTRY_ARGS[name])))))
            return self.codes.get(name, 0)
        return entry


@pytest.fixture
def standin(monkeypatch):
    """ops on the stand-in library with the thresholds down, so that a 1 x 16 x 8 x 8 layer reaches every launcher."""
    from mydetection_amd import _lib, ops
    lib = StandInLibrary(_lib.lib())
    monkeypatch.setattr(_lib, 'lib', lambda: lib)
    monkeypatch.setattr(ops, '_stream', lambda: ctypes.c_void_p(0))
    monkeypatch.setattr(ops, 'require_gpu', lambda t, what: None)
    for name, value in (('P3_MIN_WGS', 1), ('P3_MIN_FILL', 0.0), ('WINO4_MIN_ITEMS', 1), ('WINOGRAD', True), ('WINOGRAD4', True),
                        ('SPLIT_BF16', True), ('CONV_P3', True), ('TIMER', None), ('_WORKSPACE', {}), ('_WINO4_WS', {})):
        monkeypatch.setattr(ops, name, value)
    return lib


def _layer(k=3, stride=1, residual=False):
    """CPU tensors of a B = 1, 8 x 8, 16 -> 16 layer and one stand-in tensor per weight form."""
    from mydetection_amd import ops
    x, _ = ops.empty_nhwc(1, 16, 8, 8, 'cpu')
    t = dict(x=x, w=torch.zeros(16, k, k, 16), scale=torch.ones(16), shift=torch.zeros(16),
             wino=torch.zeros(4), wino4=torch.zeros(4), b3=torch.zeros(4, dtype=torch.int16))
    if residual:
        t['residual'], _ = ops.empty_nhwc(1, 16, 8 // stride, 8 // stride, 'cpu')
    return t


def _conv(t, forms, k=3, stride=1, b3_min_rows=1, **kw):
    from mydetection_amd import ops
    p = (k - 1) // 2
    return ops.conv2d(t['x'], t['w'], t['scale'], t['shift'], k, stride, (p, p, p, p), ops.ACT_LEAKY, residual=t.get('residual'),
                      b3_min_rows=b3_min_rows, **{f: t[f] for f in forms}, **kw)


ROUTES = [((), 3, 1, ('conv_igemm',)),
          (('wino',), 3, 1, ('conv_wino',)),
          (('wino4',), 3, 1, ('conv_wino4',)),
          (('wino', 'wino4'), 3, 1, ('conv_wino4',)),
          (('wino', 'b3'), 3, 1, ('conv_p3', 'conv_wino')),
          (('wino', 'wino4', 'b3'), 3, 1, ('conv_p3', 'conv_wino4')),
          (('b3',), 3, 1, ('conv_p3', 'conv_igemm_b3', 'conv_igemm')),
          (('b3',), 3, 2, ('conv_p3', 'conv_igemm_b3', 'conv_igemm')),
          (('wino', 'wino4', 'b3'), 3, 2, ('conv_p3', 'conv_igemm_b3', 'conv_igemm')),
          (('b3',), 1, 1, ('conv_igemm',)),                   # 16 output channels: below the 1x1 layers' 128
          (('wino', 'wino4'), 1, 1, ('conv_igemm',))]


@pytest.mark.parametrize('forms,k,stride,route', ROUTES)
def test_conv2d_walks_the_route(standin, forms, k, stride, route):
    """The first entry point called is the route's first launcher, with the weight form of its table row; MYDET_E_UNSUPP from it leads to
    exactly one further call, to the next launcher, with the same tensors and shape; the last launcher's refusal, and any other code from
    any of them, raises MydetError naming the entry point."""
    from mydetection_amd import _lib, ops
    t = _layer(k, stride, residual=True)
    p = (k - 1) // 2
    assert ops.conv_route(1, 8, 8, 16, 16, k, stride, (p, p, p, p), ops.ACT_LEAKY, gated=False, ldy=16, ldr=16, forms=set(forms),
                          b3_min_rows=1) == route
    entries = [ops.CONV_LAUNCHERS[f][0] for f in route]
    for n in range(len(route)):                                 # the first n launchers refuse
        standin.calls, standin.codes = [], {e: UNSUPP for e in entries[:n]}
        out, _ = ops.empty_nhwc(1, 16, 8 // stride, 8 // stride, 'cpu')
        assert _conv(t, forms, k, stride, out=out) is out
        assert [name for name, _ in standin.calls] == entries[:n + 1]
        for (name, args), family in zip(standin.calls, route):
            form = ops.CONV_LAUNCHERS[family][2]
            assert args.pop('weight') == (t[form] if form else t['w']).data_ptr(), (family, form)
            assert args == dict(x=t['x'].data_ptr(), ldx=16, scale=t['scale'].data_ptr(), shift=t['shift'].data_ptr(),
                                residual=t['residual'].data_ptr(), ldr=16, out=out.data_ptr(), ldy=16, B=1, H=8, W=8, Cin=16, Cout=16,
                                act=ops.ACT_LEAKY), name
    for n, entry in enumerate(entries):                         # launcher n fails
        for code in (-1, 700) + ((UNSUPP,) if n == len(entries) - 1 else ()):
            standin.calls, standin.codes = [], {**{e: UNSUPP for e in entries[:n]}, entry: code}
            with pytest.raises(_lib.MydetError, match=entry + ' failed'):
                _conv(t, forms, k, stride)
            assert [name for name, _ in standin.calls] == entries[:n + 1]


def test_switches_are_read_at_every_call(standin, monkeypatch):
    from mydetection_amd import ops
    t = _layer()

    def first(forms, **kw):
        standin.calls = []
        _conv(t, forms, **kw)
        return standin.calls[0][0]
    everything = ('wino', 'wino4', 'b3')
    assert first(everything) == 'mydet_conv3x3_p3_f32'
    monkeypatch.setattr(ops, 'CONV_P3', False)
    assert first(everything) == 'mydet_conv2d_wino4_f32'
    assert first(('b3',)) == 'mydet_conv2d_igemm_b3_f32'
    monkeypatch.setattr(ops, 'WINOGRAD4', False)
    assert first(everything) == 'mydet_conv2d_wino_f32'
    monkeypatch.setattr(ops, 'WINOGRAD', False)
    assert first(everything) == 'mydet_conv2d_igemm_b3_f32'
    monkeypatch.setattr(ops, 'SPLIT_BF16', False)
    assert first(everything) == 'mydet_conv2d_igemm_f32'
    monkeypatch.setattr(ops, 'SPLIT_BF16', True)
    monkeypatch.setattr(ops, 'CONV_P3', True)
    assert first(everything) == 'mydet_conv3x3_p3_f32'
    monkeypatch.setattr(ops, 'WINOGRAD', True)
    monkeypatch.setattr(ops, 'WINOGRAD4', True)
    monkeypatch.setattr(ops, 'WINO4_MIN_ITEMS', 512)
    monkeypatch.setattr(ops, 'CONV_P3', False)
    assert first(everything) == 'mydet_conv2d_wino_f32'         # a grid of one workgroup: F(2x2) where both forms are held
    assert first(('b3',), b3_min_rows=None) == 'mydet_conv2d_igemm_f32'          # 64 rows: below B3_MIN_ROWS


def test_pricing_is_one_function(standin, monkeypatch):
    """KernelTimer gets the direct form's FLOPs and input + output + weights (+ residual) bytes for every family, under the family's name;
    only conv_igemm discounts a block-interior tensor in the fused-minimum bytes."""
    from mydetection_amd import ops
    calls = []

    class Timer:
        def start(self):
            return 't0'

        def stop(self, name, t0, work=0.0, nbytes=0.0, fused=None):
            calls.append((name, work, nbytes, fused))
    monkeypatch.setattr(ops, 'TIMER', Timer())
    t = _layer(residual=True)
    work, b_in, b_out, b_w = 2.0 * 64 * 16 * 9 * 16, 4.0 * 64 * 16, 4.0 * 64 * 16, 4.0 * 9 * 16 * 16
    for forms, refuse, family in (((), (), 'conv_igemm'), (('wino',), (), 'conv_wino'), (('wino4',), (), 'conv_wino4'), (('b3',), (), 'conv_p3'),
                                  (('b3',), ('mydet_conv3x3_p3_f32',), 'conv_igemm_b3')):
        del calls[:]
        standin.codes = {e: UNSUPP for e in refuse}
        _conv(t, forms, interior='in')
        fused = b_out + b_w + b_out if family == 'conv_igemm' else None
        assert calls == [(family, work, b_in + b_out + b_w + b_out, fused)], family
    monkeypatch.setattr(ops, 'TIMER_DETAIL', True)
    del calls[:]
    standin.codes = {}
    _conv(_layer(stride=2), ('b3',), stride=2)
    assert calls[0][0] == 'conv_p3 16->16 k3s2 8x8'
    assert ops.conv_price('conv_wino4', 2, 16, 24, 16, 24, 32, 64, 3, False, 'out') == (
        2.0 * 2 * 16 * 24 * 64 * 9 * 32, 4.0 * (2 * 16 * 24 * 32 + 2 * 16 * 24 * 64 + 9 * 32 * 64), None)
