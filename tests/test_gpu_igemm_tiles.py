"""GPU: every tile configuration of the float32 implicit GEMM (conv_igemm_kernel, csrc/conv_igemm.hip) against float64.

mydet_conv2d_igemm_f32 is the kernel every other conv form falls back to; it is one template instantiated for seven tile
configurations (ids 0, 1, 2, 3, 6, 8, 9 of launch_cfg), each with aligned / generic K, three activations with and without a residual,
the squeeze-excite gate, and a K-cut tail with its own fixup kernel.  The tile rule (choose_cfg) sends the small shapes of a test
to two or three of them, so here MYDET_CONV_CFG -- read on every call -- forces each id in turn on shapes of a few hundred rows: any
shape the entry point accepts is legal for every tile.  The launch plan (which id, whether a K-cut tail ran) is not guessed: it is
asked from the launcher's own arithmetic through mydet_conv_igemm_plan.

Bound: the project's 2e-5 * max(1, max|ref|) against a float64 reference of the same operation (tests/test_gpu_kernels.py:
_conv_case), for every id and case."""
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

from _arena import arena

pytestmark = pytest.mark.gpu

IDS = (0, 1, 2, 3, 6, 8, 9)
TILES = {0: (128, 128, 32), 1: (128, 64, 32), 2: (128, 32, 32), 3: (64, 64, 32), 6: (128, 64, 16), 8: (128, 128, 32), 9: (128, 96, 32)}
WS_BYTES = 64 << 20                 # ops.WORKSPACE_BYTES: what ops.conv2d hands the launcher


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    from mydetection_amd import _lib
    _lib.lib()                                   # fail loudly if the HIP library is missing
    return torch.device('cuda:0')


def _plan(cfg, c):
    """The launcher's plan for case `c` on this device: dict(id, BM, BN, BK, main, tail, cuts)."""
    from mydetection_amd import _lib, ops
    assert ops.WORKSPACE_BYTES == WS_BYTES
    out = (ctypes.c_int32 * 7)()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    Ho, Wo = c['ref'].shape[2:]
    _lib.check(_lib.lib().mydet_conv_igemm_plan(cfg, c['B'], Ho, Wo, c['Cin'], c['Cout'], c['k'] * c['k'], WS_BYTES, cus, out),
               'mydet_conv_igemm_plan')
    p = dict(zip(('id', 'BM', 'BN', 'BK', 'main', 'tail', 'cuts'), out))
    assert (p['BM'], p['BN'], p['BK']) == TILES[p['id']] and (cfg < 0 or p['id'] == cfg), p
    return p


# name -> shape and epilogue; `kcut`: the launch must have a K-cut tail (cuts >= 2) on every tile, asserted through the plan
CASES = {
    # a. ragged M across image borders (63 pixels per image), ragged N: a nearly empty last N tile on BN = 32 / 64 / 96 / 128
    'a_ragged_mn': dict(B=3, Cin=64, Cout=132, k=1, s=1, H=7, W=9, act=1),
    # b. generic K (Cin % 32 and % 16 != 0), short: two slabs, the second mostly past K
    'b_generic_k_short': dict(B=2, Cin=40, Cout=72, k=1, s=1, H=9, W=5, act=2, residual=True),
    # c. 3x3, stride 2, asymmetric (static-SAME) pad, bias only
    'c_3x3_s2_asym_pad': dict(B=2, Cin=32, Cout=68, k=3, s=2, H=15, W=18, act=0, pad=(0, 0, 1, 1), bias_only=True),
    # d. 3x3, stride 1, pad 1, generic K (a slab straddles taps)
    'd_3x3_generic_k': dict(B=1, Cin=24, Cout=36, k=3, s=1, H=11, W=13, act=1, residual=True),
    # e. long aligned K on a small grid: cut along K as a whole, the fixup kernel applies the epilogue.  The issue's two epilogues, and
    # the other two of leaky / swish so that every ACT x RES instance of the fixup kernel runs (a swish fixup that took the residual
    # instance for the plain one reads a null residual of zero bytes -- zeros -- and is only seen WITH a residual)
    'e_kcut_leaky_res': dict(B=2, Cin=768, Cout=136, k=1, s=1, H=5, W=15, act=1, residual=True, kcut=True),
    'e_kcut_swish': dict(B=2, Cin=768, Cout=136, k=1, s=1, H=5, W=15, act=2, kcut=True),
    'e_kcut_swish_res': dict(B=2, Cin=768, Cout=136, k=1, s=1, H=5, W=15, act=2, residual=True, kcut=True),
    'e_kcut_leaky': dict(B=2, Cin=768, Cout=136, k=1, s=1, H=5, W=15, act=1, kcut=True),
    # f. long generic K with a K cut: slices start inside taps
    'f_kcut_generic_k': dict(B=1, Cin=88, Cout=88, k=3, s=1, H=10, W=10, act=0, residual=True, kcut=True),
    # g. the squeeze-excite gate on the A operand: short K, and a long K that is cut (aligned for both BK)
    'g_gate_short_k': dict(B=3, Cin=96, Cout=40, k=1, s=1, H=6, W=7, act=0, residual=True, gate=True),
    'g_gate_kcut': dict(B=3, Cin=1152, Cout=48, k=1, s=1, H=5, W=5, act=0, gate=True, kcut=True),
    # shapes the rule itself sends to 1, 8 and 9 (test_rule_reached_tiles)
    'rule_1': dict(B=2, Cin=64, Cout=64, k=1, s=1, H=9, W=11, act=1),
    'rule_8': dict(B=2, Cin=128, Cout=1024, k=1, s=1, H=9, W=11, act=2),
    'rule_9': dict(B=25, Cin=384, Cout=96, k=1, s=1, H=40, W=40, act=0, residual=True),
}


@functools.lru_cache(maxsize=None)
def _case(name):
    """Inputs (CPU, float32; randn, weights randn / sqrt(K), seeded as _conv_case does) and the float64 reference, built once."""
    c = dict(CASES[name])
    B, Cin, Cout, k, s, H, W = (c[n] for n in ('B', 'Cin', 'Cout', 'k', 's', 'H', 'W'))
    g = torch.Generator().manual_seed(sorted(CASES).index(name))
    x = torch.randn(B, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, k, k, generator=g) / (Cin * k * k) ** 0.5
    scale = None if c.get('bias_only') else torch.rand(Cout, generator=g) + 0.5
    shift = torch.randn(Cout, generator=g) * 0.1
    gate = torch.rand(B, Cin, generator=g) * 0.98 + 0.01 if c.get('gate') else None
    pad = c.get('pad') or ((k - 1) // 2,) * 4                      # (top, left, bottom, right)
    xd = x.double() * gate.double().view(B, Cin, 1, 1) if gate is not None else x.double()
    if k == 1 and s == 1:                                          # one matmul
        ref = torch.einsum('bchw,oc->bohw', xd, w.double().view(Cout, Cin))
    else:
        ref = F.conv2d(F.pad(xd, (pad[1], pad[3], pad[0], pad[2])), w.double(), None, s)
    ref = ref * (scale.double().view(1, -1, 1, 1) if scale is not None else 1.0) + shift.double().view(1, -1, 1, 1)
    if c['act'] == 1:
        ref = F.leaky_relu(ref, 0.1)
    elif c['act'] == 2:
        ref = ref * torch.sigmoid(ref)
    res = None
    if c.get('residual'):
        res = torch.randn(ref.shape, generator=g)
        ref = ref + res.double()
    c.update(x=x, w=w, scale=scale, shift=shift, gate=gate, res=res, pad=pad, ref=ref, name=name,
             tol=2e-5 * max(1.0, ref.abs().max().item()))
    return c


def _device_args(c, dev):
    return dict(x=c['x'].to(dev).contiguous(memory_format=torch.channels_last), w=c['w'].permute(0, 2, 3, 1).contiguous().to(dev),
                scale=c['scale'].to(dev) if c['scale'] is not None else None, shift=c['shift'].to(dev),
                res=c['res'].to(dev).contiguous(memory_format=torch.channels_last) if c['res'] is not None else None,
                gate=c['gate'].to(dev).contiguous() if c['gate'] is not None else None)


def _run(c, d, x=None, out=None):
    from mydetection_amd import ops
    y = ops.conv2d(d['x'] if x is None else x, d['w'], d['scale'], d['shift'], c['k'], c['s'], c['pad'], c['act'], residual=d['res'],
                   gate=d['gate'], out=out)
    torch.cuda.synchronize()
    return y


def _held(c, y, what):
    """|y - ref| against the bound; prints the figure first.  Returns error / bound."""
    assert tuple(y.shape) == tuple(c['ref'].shape)
    yc = y.cpu().double()
    assert bool(torch.isfinite(yc).all()), f'{what}: non-finite output'
    err = (yc - c['ref']).abs().max().item()
    print(f"igemm_tiles {c['name']} {what}: err {err:.3e} = {err / c['tol']:.3f} of the bound {c['tol']:.3e}")
    assert err <= c['tol'], f"{c['name']} {what}: {err} > {c['tol']}"
    return err / c['tol']


def _sweep(c, d, monkeypatch, run):
    """The checks of one case: un-forced, then every id forced.  run(cfg) -> (first result, second result) of two calls."""
    monkeypatch.delenv('MYDET_CONV_CFG', raising=False)
    rule = _plan(-1, c)
    y_rule, _ = run(None)
    _held(c, y_rule, f"rule (cfg {rule['id']})")
    for cfg in IDS:
        plan = _plan(cfg, c)
        if c.get('kcut'):           # the K-cut kernel and the fixup kernel ran, on this chip's CU count
            assert plan['cuts'] >= 2 and plan['tail'] > 0, (c['name'], plan)
        monkeypatch.setenv('MYDET_CONV_CFG', str(cfg))
        y, y2 = run(cfg)
        monkeypatch.delenv('MYDET_CONV_CFG')
        assert torch.equal(y, y2), f"{c['name']} cfg {cfg}: a second call differs"
        _held(c, y, f"cfg {cfg} ({plan['BM']}x{plan['BN']}x{plan['BK']}, {plan['main']} + {plan['tail']} x {plan['cuts']})")
        diff = (y.double() - y_rule.double()).abs().max().item()
        assert diff <= c['tol'], f"{c['name']} cfg {cfg}: differs from the un-forced call by {diff} > {c['tol']}"
        if rule['id'] == cfg:
            assert torch.equal(y, y_rule), f"{c['name']}: the rule picks cfg {cfg}, the forced call differs from the un-forced one"


SWEPT = [n for n in CASES if not n.startswith('rule_')]


@pytest.mark.parametrize('name', SWEPT)
def test_every_tile_vs_fp64(dev, monkeypatch, name):
    c = _case(name)
    d = _device_args(c, dev)
    _sweep(c, d, monkeypatch, lambda cfg: (_run(c, d), _run(c, d)))


def test_every_tile_on_views(dev, monkeypatch):
    """Case a with x a channel slice of a wider map (ldx > Cin, NaN in the channels around the slice) and y a channel slice of a
    poisoned arena (ldy > Cout): the same checks, every word of the view written, nothing outside it, and the same bits as the
    contiguous launch of that id."""
    c = _case('a_ragged_mn')
    d = _device_args(c, dev)
    B, Cin, Cout, H, W = c['B'], c['Cin'], c['Cout'], c['H'], c['W']
    xv, xchk = arena(B, Cin, H, W, Cin + 24, 8, dev, data=c['x'].to(dev))

    def run(cfg):
        ys = []
        for _ in range(2):
            out, chk = arena(B, Cout, H, W, 160, 12, dev)
            y = _run(c, d, x=xv, out=out)
            assert y.data_ptr() == out.data_ptr()
            chk.view_defined(f'conv_igemm cfg {cfg} output')
            chk.outside_untouched(f'conv_igemm cfg {cfg} output')
            ys.append(y)
        if cfg is not None:
            assert torch.equal(ys[0], _run(c, d)), f'cfg {cfg}: the launch on views differs from the contiguous one'
        return ys

    _sweep(c, d, monkeypatch, run)
    xchk.outside_untouched('conv_igemm input')


def test_forced_bad_id_is_an_error(dev, monkeypatch):
    """The control: MYDET_CONV_CFG does reach the launcher (the sweep would pass vacuously if it did not)."""
    from mydetection_amd import _lib
    c = _case('a_ragged_mn')
    d = _device_args(c, dev)
    monkeypatch.setenv('MYDET_CONV_CFG', '5')
    with pytest.raises(_lib.MydetError, match='bad argument'):
        _run(c, d)
    monkeypatch.undo()
    _held(c, _run(c, d), 'after undo')


@pytest.mark.parametrize('name,cfg', [('rule_1', 1), ('rule_8', 8), ('rule_9', 9)])
def test_rule_reached_tiles(dev, monkeypatch, name, cfg):
    """Shapes that the rule itself sends to 1, 8 and 9 (no environment): the plan says so, the result is held to float64 and is
    the forced run's, bit for bit."""
    monkeypatch.delenv('MYDET_CONV_CFG', raising=False)
    c = _case(name)
    d = _device_args(c, dev)
    plan = _plan(-1, c)
    assert plan['id'] == cfg and (plan['BM'], plan['BN'], plan['BK']) == TILES[cfg], plan
    y = _run(c, d)
    _held(c, y, f'rule (cfg {cfg})')
    monkeypatch.setenv('MYDET_CONV_CFG', str(cfg))
    yf = _run(c, d)
    monkeypatch.delenv('MYDET_CONV_CFG')
    assert torch.equal(y, yf), f'{name}: the forced run of cfg {cfg} differs from the rule-reached one'
