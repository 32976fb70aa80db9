"""GPU: every launch branch of the split-bf16 convolutions against float64 -- conv_igemm_b3_kernel and conv_igemm_b3w_kernel with
their K-cut (SPLIT) instances and conv_fixup_kernel behind them (csrc/conv_igemm.hip), and conv_p3_kernel (csrc/conv_p3.hip).

The launcher has five tile forms (128 x 64 for Cout <= 64; 64 x 128 for small grids; 128 x 128; 128 x 128 on 8 waves; 128 x 256 wide),
each with three activations with and without a residual, the squeeze-excite gate on the three 4-wave forms, and a K-cut tail with
its own fixup launch under two rules (`small`: the whole grid; `rounds 2..4`: the tiles behind the whole rounds).  The form rule sends
a test-sized shape to one or two of them, so MYDET_B3_HALF_TILES / MYDET_B3_WAVES / MYDET_B3_WIDE (re-read through
mydet_conv_b3_reload_tuning) force each in turn.  Which branch ran is not guessed: every case first asks the launcher's own arithmetic
(mydet_conv_b3_plan / mydet_conv3x3_p3_plan, with this device's CU count and ops.WORKSPACE_BYTES) and asserts the branch it is named
for; tests/test_b3_plan_host.py pins that arithmetic.  test_reached_instances lists the kernel instances the cases reach, from the
same hooks, and asserts that none the dispatch code can emit is missing.

Bounds (the project's, tests/test_gpu_kernels.py): |y - ref| <= 2e-5 * max(1, max|ref|) against a float64 reference of the whole op;
err <= 4 * err32 + 1e-6 against conv_igemm_kernel on the same inputs; two launches bit-equal.

Selection tests: the bound above is global, so it cannot see a lost small piece of an operand at a small output.  With one operand a
power of two the three pieces of the other must come through element by element: a three-piece bfloat16 split reconstructs a float32
exactly (8 + 8 + 8 bits by round-to-nearest remainders), every kept product is then exact, and the float32 sum of three
non-overlapping pieces, small ones first, rounds at most once: |y - expected| <= 2^-22 * |expected| per element, where a lost third
piece costs 2^-16.  The bound is checked first on a CPU emulation of the split on the very inputs (_selection).  Of the six kept
products (activation piece, weight piece) = (2,0) (1,1) (0,2) (1,0) (0,1) (0,0), one-hot weights see (2,0) (1,0) (0,0) and one-hot
activations (0,2) (0,1) (0,0); (1,1) is zero whenever one operand is a power of two, so only the dense cases see it -- through
err <= 4 * err32 + 1e-6.  (Tried on scratch builds: without (2,0), or without (0,2), every selection test of that kind fails, on every
form and geometry; without (1,1) none of them does and 70 dense cases do; with the RES instances of the swish fixup line swapped,
the ten swish K-cut cases fail and nothing else.)"""
import contextlib
import functools
import itertools
import zlib

import pytest
import torch
import torch.nn.functional as F

from _arena import arena

pytestmark = pytest.mark.gpu

HALF, WAVES, WIDE = 'MYDET_B3_HALF_TILES', 'MYDET_B3_WAVES', 'MYDET_B3_WIDE'
# form -> the switches that force it, the reload's form bits, the plan's (form, BM, BN, WN), and which of a shape's three Cout it takes
FORMS = {
    't64': dict(env={}, bits=0, tile=(0, 128, 64, 2), cout=0),                                   # Cout <= 64, default switches
    'half': dict(env={HALF: str(1 << 30)}, bits=0, tile=(0, 64, 128, 2), cout=1),
    't128': dict(env={HALF: '0'}, bits=0, tile=(0, 128, 128, 2), cout=1),
    'waves8': dict(env={HALF: '0', WAVES: '8'}, bits=2, tile=(2, 128, 128, 4), cout=1),
    'wide': dict(env={HALF: '0', WIDE: '1'}, bits=1, tile=(1, 128, 256, 4), cout=2),             # Cout > 192
}
GATED_FORMS = ('t64', 'half', 't128')
ACT_NONE, ACT_LEAKY, ACT_SWISH = 0, 1, 2
EPILOGUES = tuple(itertools.product((ACT_NONE, ACT_LEAKY, ACT_SWISH), (False, True)))          # (act, residual)
# cout: (for 't64', for the 128-wide forms, for 'wide'); None: the form does not take the shape.  kcut: `small` K-cut tail on every form
SHAPES = {
    # ragged M across image borders (63 pixels per image), ragged N: 4 live channels in the last 128- / 256-wide tile
    'a_ragged_mn': dict(B=3, Cin=64, k=1, s=1, H=7, W=9, cout=(36, 132, 260)),
    # Cin % 16 == 8 on a 1x1 layer: the last slab half zeros (the wide form has no such instance: test_refusals)
    'b_cin40': dict(B=2, Cin=40, k=1, s=1, H=9, W=5, cout=(40, 72, None)),
    # 3x3, stride 2, asymmetric (static-SAME) pad, bias only
    'c_3x3_s2_asym_pad': dict(B=2, Cin=32, k=3, s=2, H=15, W=18, pad=(0, 0, 1, 1), bias_only=True, cout=(44, 68, 196)),
    # 3x3, stride 1, pad 1
    'd_3x3_s1': dict(B=1, Cin=16, k=3, s=1, H=11, W=13, cout=(36, 68, 196)),
    # long K on a small grid: cut along K as a whole (`small`), 1x1 (48 slabs) and 3x3 (36 slabs)
    'e_kcut': dict(B=2, Cin=768, k=1, s=1, H=5, W=15, cout=(48, 136, 264), kcut=True),
    'e_kcut_3x3': dict(B=2, Cin=64, k=3, s=1, H=5, W=15, cout=(48, 136, 264), kcut=True),
    # the squeeze-excite gate on the A operand, short K and a K that is cut
    'g_gate': dict(B=3, Cin=96, k=1, s=1, H=6, W=7, gated=True, cout=(40, 72, None)),
    'g_gate_kcut': dict(B=3, Cin=1152, k=1, s=1, H=5, W=5, gated=True, cout=(48, 136, None), kcut=True),
}
PLAIN = ('a_ragged_mn', 'b_cin40', 'c_3x3_s2_asym_pad', 'd_3x3_s1')
KCUT = ('e_kcut', 'e_kcut_3x3')
GATE = ('g_gate', 'g_gate_kcut')


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    from mydetection_amd import _lib
    _lib.lib()                                   # fail loudly if the HIP library is missing
    return torch.device('cuda:0')


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


@contextlib.contextmanager
def _form(monkeypatch, form):
    """The launcher under the switches of `form` (read once per process otherwise); back at the default on the way out."""
    from mydetection_amd import _lib
    for name in (HALF, WAVES, WIDE):
        monkeypatch.delenv(name, raising=False)
    for name, value in FORMS[form]['env'].items():
        monkeypatch.setenv(name, value)
    assert _lib.lib().mydet_conv_b3_reload_tuning() == FORMS[form]['bits']
    try:
        yield
    finally:
        monkeypatch.undo()
        assert _lib.lib().mydet_conv_b3_reload_tuning() == 0


def _cout(shape, form):
    return SHAPES[shape]['cout'][FORMS[form]['cout']]


def _geometry(c):
    k, s = c['k'], c['s']
    pad = c.get('pad') or ((k - 1) // 2,) * 4                      # (top, left, bottom, right)
    Ho = (c['H'] + pad[0] + pad[2] - k) // s + 1
    Wo = (c['W'] + pad[1] + pad[3] - k) // s + 1
    return pad, Ho, Wo


def _plan(c, Cout, form=None):
    """The launcher's plan for shape `c` with Cout channels under the switches in force; with `form`: it is that form's tile."""
    from mydetection_amd import ops
    _, Ho, Wo = _geometry(c)
    p = ops.b3_plan(c['B'], Ho, Wo, c['Cin'], Cout, c['k'] * c['k'], gated=bool(c.get('gated')), workspace_bytes=ops.WORKSPACE_BYTES,
                    cus=_cus())
    assert isinstance(p, ops.B3Plan), (c, Cout, p)
    if form is not None:
        assert (p.form, p.bm, p.bn, p.wn) == FORMS[form]['tile'], (form, c, Cout, p)
    total = -(-c['B'] * Ho * Wo // p.bm) * -(-Cout // p.bn)
    assert p.main + p.tail == total and (p.tail > 0) == (p.cuts >= 2), p
    if c.get('kcut'):
        assert p.tail > 0 and p.cuts >= 2, (form, c, Cout, p)
    else:
        assert p.tail == 0 and p.main == total, (form, c, Cout, p)
    return p


@functools.lru_cache(maxsize=None)
def _base(shape, Cout):
    """Inputs (CPU, float32; randn, weights randn / sqrt(K)) and the float64 conv * scale + shift of the gated input, built once."""
    c = dict(SHAPES[shape])
    B, Cin, k, s, H, W = (c[n] for n in ('B', 'Cin', 'k', 's', 'H', 'W'))
    g = torch.Generator().manual_seed(1000 * sorted(SHAPES).index(shape) + Cout)
    x = torch.randn(B, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, k, k, generator=g) / (Cin * k * k) ** 0.5
    scale = None if c.get('bias_only') else torch.rand(Cout, generator=g) + 0.5
    shift = torch.randn(Cout, generator=g) * 0.1
    gate = torch.rand(B, Cin, generator=g) * 0.98 + 0.01 if c.get('gated') else None
    pad, Ho, Wo = _geometry(c)
    xd = x.double() * gate.double().view(B, Cin, 1, 1) if gate is not None else x.double()
    pre = F.conv2d(F.pad(xd, (pad[1], pad[3], pad[0], pad[2])), w.double(), None, s)
    pre = pre * (scale.double().view(1, -1, 1, 1) if scale is not None else 1.0) + shift.double().view(1, -1, 1, 1)
    assert tuple(pre.shape) == (B, Cout, Ho, Wo)
    res = torch.randn(pre.shape, generator=g)
    c.update(name=f'{shape}/{Cout}', Cout=Cout, x=x, w=w, scale=scale, shift=shift, gate=gate, res=res, pad=pad, Ho=Ho, Wo=Wo, pre=pre)
    return c


def _activate(pre, act):
    return F.leaky_relu(pre, 0.1) if act == ACT_LEAKY else pre * torch.sigmoid(pre) if act == ACT_SWISH else pre


@functools.lru_cache(maxsize=None)
def _ref(shape, Cout, act, residual):
    """(float64 reference of the whole op, the bound)."""
    c = _base(shape, Cout)
    ref = _activate(c['pre'], act)
    if residual:
        ref = ref + c['res'].double()
    return ref, 2e-5 * max(1.0, ref.abs().max().item())


_DEVICE = {}


def _device_args(c, dev):
    """The operands of a case on the device, uploaded (and the weight split) once."""
    from mydetection_amd import ops
    if c['name'] not in _DEVICE:
        w = c['w'].permute(0, 2, 3, 1).contiguous().to(dev)
        w3 = ops.split_bf16(w)
        assert w3 is not None
        _DEVICE[c['name']] = dict(x=c['x'].to(dev).contiguous(memory_format=torch.channels_last), w=w, w3=w3,
                                  scale=c['scale'].to(dev) if c['scale'] is not None else None, shift=c['shift'].to(dev),
                                  res=c['res'].to(dev).contiguous(memory_format=torch.channels_last),
                                  gate=c['gate'].to(dev).contiguous() if c['gate'] is not None else None)
    return _DEVICE[c['name']]


def _b3(c, d, act, residual, x=None, out=None, res=None, w3=None, gate=True):
    """mydet_conv2d_igemm_b3_f32 itself (ops.conv2d sends only some layers to it): (return code, output)."""
    from mydetection_amd import _lib, ops
    x, ldx = ops.to_nhwc(d['x'] if x is None else x)
    B, Cin, H, W = x.shape
    if out is None:
        out, ldy = ops.empty_nhwc(B, c['Cout'], c['Ho'], c['Wo'], x.device)
    else:
        ldy = ops.nhwc_ld(out)
        assert ldy is not None and tuple(out.shape) == (B, c['Cout'], c['Ho'], c['Wo'])
    r, ldr = (None, 0)
    if residual:
        r, ldr = ops.to_nhwc(d['res'] if res is None else res)
    ws = ops.conv_workspace(x.device)
    p = ops._ptr
    rc = _lib.lib().mydet_conv2d_igemm_b3_f32(p(x), ldx, p(d['w3'] if w3 is None else w3), p(d['scale']), p(d['shift']), p(r), ldr,
                                              p(d['gate'] if gate else None), p(ws), ws.numel() * 4, p(out), ldy, B, H, W, Cin,
                                              c['Cout'], c['k'], c['k'], c['s'], c['pad'][0], c['pad'][1], c['Ho'], c['Wo'], act,
                                              ops._stream())
    return rc, out


_ERR32 = {}


def _err32(c, d, shape, act, residual):
    """Error of conv_igemm_kernel (the float32-instruction kernel) on the same inputs, once per case and epilogue."""
    from mydetection_amd import ops
    key = (c['name'], act, residual)
    if key not in _ERR32:
        y32 = ops.conv2d(d['x'], d['w'], d['scale'], d['shift'], c['k'], c['s'], c['pad'], act, residual=d['res'] if residual else None,
                         gate=d['gate'])
        _ERR32[key] = (y32.cpu().double() - _ref(shape, c['Cout'], act, residual)[0]).abs().max().item()
    return _ERR32[key]


def _held(c, d, shape, act, residual, what, y=None):
    """One epilogue of one case: two launches bit-equal, held to float64 and to the float32 kernel's error.  Returns the output."""
    ref, tol = _ref(shape, c['Cout'], act, residual)
    if y is None:
        rc, y = _b3(c, d, act, residual)
        rc2, y2 = _b3(c, d, act, residual)
        torch.cuda.synchronize()
        assert rc == 0 and rc2 == 0, (what, rc, rc2)
        assert torch.equal(y, y2), f'{what}: a second launch differs'
    yc = y.cpu().double()
    assert tuple(yc.shape) == tuple(ref.shape) and bool(torch.isfinite(yc).all()), what
    err = (yc - ref).abs().max().item()
    e32 = _err32(c, d, shape, act, residual)
    print(f'b3_branches {what} act {act} res {int(residual)}: err {err:.3e} = {err / tol:.3f} of the bound {tol:.3e}; float32 kernel {e32:.3e}')
    assert err <= tol, f'{what} act {act} res {residual}: {err} > {tol}'
    assert err <= 4.0 * e32 + 1e-6, f'{what} act {act} res {residual}: split-bf16 error {err:.2e} vs float32-instruction error {e32:.2e}'
    return y


def _plan_text(p):
    return f'{p.bm}x{p.bn} wn{p.wn} form {p.form}, {p.main} + {p.tail} x {p.cuts}'


# ---------------------------------------------------------------------------------------------------------------- conv_igemm_b3 / b3w

@pytest.mark.parametrize('form,shape', [(f, n) for f in FORMS for n in PLAIN + KCUT if SHAPES[n]['cout'][FORMS[f]['cout']] is not None])
def test_every_form_and_epilogue_vs_fp64(dev, monkeypatch, form, shape):
    """Each form on each shape, all six ACT x RES epilogues.  On the `kcut` shapes the whole grid is cut along K: the SPLIT instance
    writes partial tiles and conv_fixup_kernel<BM, BN, 2, WN, ACT, RES> applies the epilogue (a fixup that took the wrong RES instance
    shows only with a residual; the plain ACT_NONE one is here too, so that every instance the launcher can emit runs)."""
    Cout = _cout(shape, form)               # (b_cin40 not on the wide form: it has no Cin % 16 != 0 instance, test_refusals)
    c = _base(shape, Cout)
    d = _device_args(c, dev)
    with _form(monkeypatch, form):
        p = _plan(c, Cout, form)
        for act, residual in EPILOGUES:
            _held(c, d, shape, act, residual, f'{form} {c["name"]} ({_plan_text(p)})')


@pytest.mark.parametrize('shape', GATE)
@pytest.mark.parametrize('form', GATED_FORMS)
def test_gate_vs_fp64(dev, monkeypatch, form, shape):
    """The squeeze-excite gate (GATE instances: the activations are multiplied per image and channel before they are split), with and
    without a residual; on the long K the gated SPLIT instance and the fixup."""
    Cout = _cout(shape, form)
    c = _base(shape, Cout)
    d = _device_args(c, dev)
    with _form(monkeypatch, form):
        p = _plan(c, Cout, form)
        for residual in (False, True):
            _held(c, d, shape, ACT_NONE, residual, f'{form} {c["name"]} gated ({_plan_text(p)})')


@pytest.mark.parametrize('form', FORMS)
def test_every_form_on_views(dev, monkeypatch, form):
    """Shape a with x a channel slice of a wider map (ldx > Cin, NaN in the channels around it), y a channel slice of a poisoned arena
    (ldy > Cout) and the residual likewise (ldr > Cout, another stride): every word of the view written, nothing outside it, and the
    bits of the contiguous launch.  Leaky with a residual, and the 3x3 stride-2 shape (its own address arithmetic) the same way."""
    for shape in ('a_ragged_mn', 'c_3x3_s2_asym_pad'):
        Cout = _cout(shape, form)
        c = _base(shape, Cout)
        d = _device_args(c, dev)
        B, Cin, H, W, Ho, Wo = c['B'], c['Cin'], c['H'], c['W'], c['Ho'], c['Wo']
        xv, xchk = arena(B, Cin, H, W, Cin + 24, 8, dev, data=d['x'])
        rv, rchk = arena(B, Cout, Ho, Wo, Cout + 20, 4, dev, data=d['res'])
        with _form(monkeypatch, form):
            _plan(c, Cout, form)
            rc, y0 = _b3(c, d, ACT_LEAKY, True)
            assert rc == 0
            for _ in range(2):
                out, chk = arena(B, Cout, Ho, Wo, Cout + 28, 12, dev)
                rc, y = _b3(c, d, ACT_LEAKY, True, x=xv, out=out, res=rv)
                torch.cuda.synchronize()
                assert rc == 0 and y.data_ptr() == out.data_ptr()
                chk.view_defined(f'conv_igemm_b3 {form} {shape} output')
                chk.outside_untouched(f'conv_igemm_b3 {form} {shape} output')
                assert torch.equal(y, y0), f'{form} {shape}: the launch on views differs from the contiguous one'
            _held(c, d, shape, ACT_LEAKY, True, f'{form} {c["name"]} on views', y=y)
        xchk.outside_untouched('conv_igemm_b3 input')
        rchk.outside_untouched('conv_igemm_b3 residual')


def test_kcut_tail_behind_whole_rounds(dev, monkeypatch):
    """The `rounds 2..4` rule, default switches, 128 x 128 tiles: 1x1, 1024 -> 128 on 136 220 rows = 1 065 row tiles (the last one a
    fifth full): two rounds of 2 x CUs workgroups in the main launch, 41 tiles cut 8 ways along K behind them, leaky with a residual.
    Inputs and the float64 reference are built on the device (the only case above a few thousand rows)."""
    from mydetection_amd import ops
    B, H, W, Cin, Cout = 7, 139, 140, 1024, 128
    c = dict(B=B, Cin=Cin, k=1, s=1, H=H, W=W, Cout=Cout, Ho=H, Wo=W, pad=(0, 0, 0, 0), kcut=True, name='rounds')
    g = torch.Generator(device=dev).manual_seed(41)
    xb = torch.randn(B, H, W, Cin, generator=g, device=dev)
    w = torch.randn(Cout, Cin, generator=g, device=dev) / Cin ** 0.5
    scale, shift = torch.rand(Cout, generator=g, device=dev) + 0.5, torch.randn(Cout, generator=g, device=dev) * 0.1
    rb = torch.randn(B, H, W, Cout, generator=g, device=dev)
    ref = F.leaky_relu(torch.matmul(xb.view(-1, Cin).double(), w.double().t()) * scale.double() + shift.double(), 0.1) + rb.view(-1, Cout).double()
    tol = 2e-5 * max(1.0, ref.abs().max().item())
    wd = w.view(Cout, 1, 1, Cin).contiguous()
    d = dict(x=xb.permute(0, 3, 1, 2), w=wd, w3=ops.split_bf16(wd), scale=scale, shift=shift, res=rb.permute(0, 3, 1, 2), gate=None)
    with _form(monkeypatch, 't64'):                        # (no switch set)
        p = _plan(c, Cout)
        cus = _cus()
        assert (p.form, p.bm, p.bn, p.wn) == (0, 128, 128, 2) and p.main == 2 * (2 * cus) and p.tail == 1065 - p.main and p.cuts >= 2, p
        assert cus != 256 or (p.tail, p.cuts) == (41, 8), p
        rc, y = _b3(c, d, ACT_LEAKY, True)
        rc2, y2 = _b3(c, d, ACT_LEAKY, True)
        torch.cuda.synchronize()
    assert rc == 0 and rc2 == 0 and torch.equal(y, y2)
    err = (y.permute(0, 2, 3, 1).reshape(-1, Cout).double() - ref).abs().max().item()
    y32 = ops.conv2d(d['x'], wd, scale, shift, 1, 1, (0, 0, 0, 0), ACT_LEAKY, residual=d['res'])
    e32 = (y32.permute(0, 2, 3, 1).reshape(-1, Cout).double() - ref).abs().max().item()
    print(f'b3_branches rounds ({_plan_text(p)}): err {err:.3e} = {err / tol:.3f} of the bound {tol:.3e}; float32 kernel {e32:.3e}')
    assert err <= tol and err <= 4.0 * e32 + 1e-6, (err, tol, e32)


def test_refusals(dev, monkeypatch):
    """By return code, nothing launched, the output arena untouched: a gate with an activation (MYDET_E_UNSUPP), the wide form with
    Cin % 16 and more than 192 output channels (MYDET_E_UNSUPP).  A gate under the 8-wave switch is no refusal: the plan shows the
    default form, and that is what runs."""
    from mydetection_amd import ops

    def refused(c, d, act, code, what, **kw):
        out, chk = arena(c['B'], c['Cout'], c['Ho'], c['Wo'], c['Cout'] + 12, 4, dev)
        rc, _ = _b3(c, d, act, False, out=out, **kw)
        torch.cuda.synchronize()
        assert rc == code, (what, rc)
        assert chk.undefined_in_view()[0] == out.numel(), f'{what}: the refused call wrote into its output'
        chk.outside_untouched(what)

    for form in GATED_FORMS:
        c = _base('g_gate', _cout('g_gate', form))
        d = _device_args(c, dev)
        with _form(monkeypatch, form):
            for act in (ACT_LEAKY, ACT_SWISH):
                refused(c, d, act, -2, f'{form}: gate with activation {act}')
    c = _base('g_gate', 72)
    d = _device_args(c, dev)
    with _form(monkeypatch, 'waves8'):
        p = _plan(c, 72)
        assert (p.form, p.bm, p.bn, p.wn) == FORMS['t128']['tile'], p
        assert (ops.b3_plan(c['B'], c['Ho'], c['Wo'], c['Cin'], 72, 1, gated=False, cus=_cus())[:4]) == FORMS['waves8']['tile']
        y8 = _held(c, d, 'g_gate', ACT_NONE, True, 'gate under MYDET_B3_WAVES=8')
        for act in (ACT_LEAKY, ACT_SWISH):
            refused(c, d, act, -2, f'waves8: gate with activation {act}')
    with _form(monkeypatch, 't128'):
        assert torch.equal(_b3(c, d, ACT_NONE, True)[1], y8), 'the gated launch under MYDET_B3_WAVES=8 is not the default form'
    c = dict(_base('b_cin40', 72), Cout=260)                 # Cin = 40 with 260 output channels: the operands of the refused call are never read
    d = _device_args(_base('b_cin40', 72), dev)
    with _form(monkeypatch, 'wide'):
        assert ops.b3_plan(c['B'], c['Ho'], c['Wo'], 40, 260, 1, cus=_cus()) == -2
        refused(c, d, ACT_LEAKY, -2, 'wide form, Cin % 16 != 0', gate=False)
        assert ops.b3_plan(c['B'], c['Ho'], c['Wo'], 40, 192, 1, cus=_cus())[:4] == FORMS['t128']['tile']       # up to 192 channels: 128 x 128


# ------------------------------------------------------------------------------------------------------------------------ conv_p3

# geometry -> (stride, H, W, strip the plan must report).  Stride 2: Ho = (H - 1) / 2 + 1, Wo likewise
P3_GEOMETRY = {
    's1': (1, 11, 19, 0),                       # 2 x 2 tiles of 8 x 16, both ragged
    's2_wo9': (2, 21, 17, 0),                   # 11 x 9: a remainder of 9 columns is a ragged 8 x 16 column
    's2_wo27': (2, 13, 53, 0),                  # 7 x 27: one whole column + a ragged one of 11
    's2_strip1': (2, 33, 47, 1),                # 17 x 24: one column + 16 x 8 strips, the second strip holds one row
    's2_strip2_wo20': (2, 65, 40, 2),           # 33 x 20: one column + 32 x 4 strips, the second strip holds one row
    's2_strip2_wo4': (2, 65, 8, 2),             # 33 x 4: no whole tile at all, strips only
}
P3_EPILOGUES = tuple(itertools.product((ACT_NONE, ACT_LEAKY), (False, True)))
# the edges: (name, B, stride, H, W, Cin, Cout)
P3_EDGES = [
    ('b1', 1, 2, 9, 9, 32, 40), ('b1_s1', 1, 1, 9, 9, 32, 136),
    ('h1_s1', 2, 1, 1, 19, 32, 40), ('h1_s2', 2, 2, 1, 19, 32, 40), ('w1_s1', 2, 1, 11, 1, 32, 40), ('w1_s2', 2, 2, 11, 1, 32, 40),
    ('h1w1_s1', 2, 1, 1, 1, 32, 136), ('h1w1_s2', 2, 2, 1, 1, 32, 136),
    ('h2w2_s2', 2, 2, 2, 2, 32, 40),                                       # Ho = Wo = 1
    ('cin16_s1', 2, 1, 11, 19, 16, 40), ('cin16_s2', 2, 2, 33, 47, 16, 136),    # one slab: the three-tap-ahead weight prefetch runs past it on every tap
    ('cout8', 2, 2, 21, 17, 32, 8), ('cout33', 2, 2, 33, 47, 32, 33),      # 33: a wave's 32-channel block with one live channel
    ('cout129_s1', 2, 1, 11, 19, 32, 129), ('cout129_s2', 2, 2, 65, 40, 32, 129),
]


def _p3_plan(Ho, Wo, Cout, stride, strip=None):
    from mydetection_amd import ops
    p = ops.p3_plan(Ho, Wo, Cout, stride)
    assert p.bn == (128 if Cout > 64 else 64), p
    if strip is not None:
        assert p.strip == strip, (Ho, Wo, Cout, stride, p)
    return p


@functools.lru_cache(maxsize=None)
def _p3_base(B, s, H, W, Cin, Cout):
    g = torch.Generator().manual_seed(7 * H + 3 * W + Cin + Cout + s)
    x = torch.randn(B, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / (Cin * 9) ** 0.5
    scale, shift = torch.rand(Cout, generator=g) + 0.5, torch.randn(Cout, generator=g) * 0.1
    pre = F.conv2d(F.pad(x.double(), (1, 1, 1, 1)), w.double(), None, s) * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1)
    assert tuple(pre.shape[2:]) == ((H - 1) // s + 1, (W - 1) // s + 1)
    return dict(x=x, w=w, scale=scale, shift=shift, pre=pre, res=torch.randn(pre.shape, generator=g), s=s, Cout=Cout)


def _p3_device(c, dev):
    from mydetection_amd import ops
    wd = c['w'].permute(0, 2, 3, 1).contiguous().to(dev)
    return dict(x=c['x'].to(dev).contiguous(memory_format=torch.channels_last), w=wd, w3=ops.split_bf16(wd), scale=c['scale'].to(dev),
                shift=c['shift'].to(dev), res=c['res'].to(dev).contiguous(memory_format=torch.channels_last))


def _p3_held(c, d, act, residual, what, x=None, out=None, res=None):
    """One epilogue of one conv_p3 case: two launches bit-equal (the second into `out` when given), float64, the float32 kernel."""
    from mydetection_amd import ops
    r = (d['res'] if res is None else res) if residual else None
    xs = d['x'] if x is None else x
    y = ops.conv3x3_p3(xs, d['w3'], d['scale'], d['shift'], c['s'], act, residual=r, cout=c['Cout'])
    y2 = ops.conv3x3_p3(xs, d['w3'], d['scale'], d['shift'], c['s'], act, residual=r, out=out, cout=c['Cout'])
    torch.cuda.synchronize()
    assert y is not None and y2 is not None and torch.equal(y, y2), f'{what}: a second launch differs'
    ref = _activate(c['pre'], act) + (c['res'].double() if residual else 0.0)
    tol = 2e-5 * max(1.0, ref.abs().max().item())
    y32 = ops.conv2d(d['x'], d['w'], d['scale'], d['shift'], 3, c['s'], (1, 1, 1, 1), act, residual=d['res'] if residual else None)
    yc = y.cpu().double()
    assert tuple(yc.shape) == tuple(ref.shape) and bool(torch.isfinite(yc).all()), what
    err, e32 = (yc - ref).abs().max().item(), (y32.cpu().double() - ref).abs().max().item()
    print(f'b3_branches p3 {what} act {act} res {int(residual)}: err {err:.3e} = {err / tol:.3f} of the bound {tol:.3e}; float32 kernel {e32:.3e}')
    assert err <= tol, f'{what}: {err} > {tol}'
    assert err <= 4.0 * e32 + 1e-6, f'{what}: split-bf16 error {err:.2e} vs float32-instruction error {e32:.2e}'
    return y


@pytest.mark.parametrize('Cout', (40, 136))
@pytest.mark.parametrize('geometry', P3_GEOMETRY)
def test_p3_every_instance_vs_fp64(dev, geometry, Cout):
    """The 32 instances of p3_dispatch: {stride 1; stride 2 x strip 0 / 1 / 2} x BN 64 / 128 x ACT none / leaky x RES, Cin = 32."""
    s, H, W, strip = P3_GEOMETRY[geometry]
    c = _p3_base(2, s, H, W, 32, Cout)
    _p3_plan(c['pre'].shape[2], c['pre'].shape[3], Cout, s, strip)
    d = _p3_device(c, dev)
    for act, residual in P3_EPILOGUES:
        _p3_held(c, d, act, residual, f'{geometry} Cout {Cout}')


@pytest.mark.parametrize('edge', P3_EDGES, ids=[e[0] for e in P3_EDGES])
def test_p3_edges_vs_fp64(dev, edge):
    name, B, s, H, W, Cin, Cout = edge
    c = _p3_base(B, s, H, W, Cin, Cout)
    _p3_plan(c['pre'].shape[2], c['pre'].shape[3], Cout, s)
    d = _p3_device(c, dev)
    for act, residual in ((ACT_LEAKY, True), (ACT_NONE, False)):
        _p3_held(c, d, act, residual, name)


@pytest.mark.parametrize('geometry', ('s1', 's2_strip1'))
def test_p3_on_views(dev, geometry):
    """One case per stride inside poisoned arenas: the input a channel slice (ldx > Cin), padded ldy and ldr (different ones)."""
    s, H, W, strip = P3_GEOMETRY[geometry]
    Cout = 136
    c = _p3_base(2, s, H, W, 32, Cout)
    Ho, Wo = c['pre'].shape[2:]
    _p3_plan(Ho, Wo, Cout, s, strip)
    d = _p3_device(c, dev)
    xv, xchk = arena(2, 32, H, W, 32 + 24, 8, dev, data=d['x'])
    rv, rchk = arena(2, Cout, Ho, Wo, Cout + 20, 4, dev, data=d['res'])
    out, chk = arena(2, Cout, Ho, Wo, Cout + 28, 12, dev)
    y = _p3_held(c, d, ACT_LEAKY, True, f'{geometry} on views', x=xv, out=out, res=rv)
    chk.view_defined('conv_p3 output')
    chk.outside_untouched('conv_p3 output')
    xchk.outside_untouched('conv_p3 input')
    rchk.outside_untouched('conv_p3 residual')
    assert torch.equal(out, y)
    y0 = _p3_held(c, d, ACT_LEAKY, True, f'{geometry} contiguous')
    assert torch.equal(y, y0), 'the launch on views differs from the contiguous one'


def test_p3_swish_is_declined(dev):
    """ops.conv3x3_p3 with ACT_SWISH returns None (the launcher: MYDET_E_UNSUPP) and writes nothing."""
    from mydetection_amd import ops
    c = _p3_base(2, 2, 21, 17, 32, 40)
    d = _p3_device(c, dev)
    Ho, Wo = c['pre'].shape[2:]
    for residual in (None, d['res']):
        out, chk = arena(2, 40, Ho, Wo, 52, 4, dev)
        assert ops.conv3x3_p3(d['x'], d['w3'], d['scale'], d['shift'], 2, ACT_SWISH, residual=residual, out=out) is None
        torch.cuda.synchronize()
        assert chk.undefined_in_view()[0] == out.numel(), 'the declined call wrote into its output'
        chk.outside_untouched('conv_p3 swish')


# ------------------------------------------------------------------------------------------------------------------ selection tests

def _full_mantissa(shape, g, emin=-20, emax=20):
    """float32 values with all 24 mantissa bits random, random sign, exponents uniform over [emin, emax]."""
    m = torch.randint(0, 1 << 23, shape, generator=g).double() / (1 << 23) + 1.0
    e = torch.randint(emin, emax + 1, shape, generator=g).double()
    sgn = torch.randint(0, 2, shape, generator=g).double() * 2 - 1
    v = (sgn * m * torch.pow(torch.tensor(2.0, dtype=torch.float64), e)).float()
    assert bool((v.double().abs() >= 2.0 ** emin).all())
    return v


def _pow2(shape, g, emin=-6, emax=6):
    e = torch.randint(emin, emax + 1, shape, generator=g).double()
    sgn = torch.randint(0, 2, shape, generator=g).double() * 2 - 1
    return (sgn * torch.pow(torch.tensor(2.0, dtype=torch.float64), e)).float()


def _pieces(v):
    """The three bfloat16 pieces of split3 (csrc/split_bf16.h), round-to-nearest-even, as float32."""
    p0 = v.bfloat16().float()
    r1 = v - p0
    p1 = r1.bfloat16().float()
    p2 = (r1 - p1).bfloat16().float()
    return p0, p1, p2


@functools.lru_cache(maxsize=None)
def _selection(kind, B, Cin, Cout, k, s, H, W, pad):
    """Inputs whose every output is ONE product of a full-mantissa operand and a power of two (or 0 in the padding).
    kind 'w': one-hot weights -- every output channel has one nonzero weight +-2^e, e in [-6, 6], at a seeded (tap, cin); the
    activations have full mantissas and exponents over [-20, 20].
    kind 'x': the mirror image -- one nonzero power of two per pixel in a seeded channel, full-mantissa weights.  Under a 3x3 window
    the nonzero pixels lie on a period-3 lattice, so that every window holds exactly one of them (possibly in the padding): with one
    per pixel an output would be a sum of nine products and the derived bound would not apply.  A 1x1 layer has one at every pixel.
    Returns (x, w, expected float64), after confirming on a CPU emulation of the split that the bound 2^-22 |expected| is met."""
    g = torch.Generator().manual_seed(zlib.crc32(repr((kind, B, Cin, Cout, k, s, H, W)).encode()))
    if kind == 'w':
        x = _full_mantissa((B, Cin, H, W), g)
        w = torch.zeros(Cout, Cin, k * k)
        w[torch.arange(Cout), torch.randint(0, Cin, (Cout,), generator=g), torch.randint(0, k * k, (Cout,), generator=g)] = _pow2((Cout,), g)
        w = w.view(Cout, Cin, k, k)
    else:
        w = _full_mantissa((Cout, Cin, k, k), g)
        ch = torch.randint(0, Cin, (B, H, W), generator=g)
        x = torch.zeros(B, Cin, H, W).scatter_(1, ch.unsqueeze(1), _pow2((B, 1, H, W), g))
        if k == 3:
            lattice = ((torch.arange(H) % 3 == 1).view(H, 1) & (torch.arange(W) % 3 == 2).view(1, W)).float()
            x = x * lattice
    conv = lambda a, b: F.conv2d(F.pad(a.double(), (pad[1], pad[3], pad[0], pad[2])), b.double(), None, s)      # noqa: E731
    expected = conv(x, w)
    assert float((expected != 0).double().mean()) > (0.5 if kind == 'w' or k == 1 else 0.05)
    # ---- the emulation: the full operand in three pieces that add up to it (2^-24: exactly, in fact), all normal numbers; the three
    # kept products that are not zero, each exact, summed in float32 small ones first as the accumulator does
    full = x if kind == 'w' else w
    p0, p1, p2 = _pieces(full)
    assert bool(((p0.double() + p1.double() + p2.double() - full.double()).abs() <= 2.0 ** -24 * full.double().abs()).all())
    for p in (p0, p1, p2):
        assert bool(((p == 0) | (p.abs() >= 2.0 ** -100)).all())
    part = [conv(p, w) if kind == 'w' else conv(x, p) for p in (p2, p1, p0)]
    assert all(bool((q.float().double() == q).all()) for q in part)
    emulated = ((part[0].float() + part[1].float()) + part[2].float()).double()
    assert bool(((emulated - expected).abs() <= 2.0 ** -22 * expected.abs()).all())
    lost = (part[1].float() + part[2].float()).double()            # (and the bound does see a lost third piece)
    assert not bool(((lost - expected).abs() <= 2.0 ** -22 * expected.abs()).all())
    return x, w, expected


def _selected(y, expected, what):
    yc = y.cpu().double()
    bad = (yc - expected).abs() > 2.0 ** -22 * expected.abs()
    rel = ((yc - expected).abs() / expected.abs().clamp_min(1e-300))[expected != 0].max().item()
    print(f'b3_branches selection {what}: max relative error 2^{torch.log2(torch.tensor(max(rel, 1e-30))).item():.1f}, '
          f'{int((expected == 0).sum())} outputs in the padding')
    assert not bool(bad.any()), (f'{what}: {int(bad.sum())} of {bad.numel()} outputs miss 2^-22 |expected|; first (b, channel, y, x): '
                                 f'{bad.nonzero()[:4].tolist()}')


SEL_SHAPES = {'1x1': dict(B=3, Cin=64, k=1, s=1, H=7, W=9, cout=(36, 132, 260)),
              '3x3': dict(B=3, Cin=32, k=3, s=1, H=7, W=9, cout=(36, 132, 260))}


@pytest.mark.parametrize('kind', ('w', 'x'))
@pytest.mark.parametrize('shape', SEL_SHAPES)
@pytest.mark.parametrize('form', FORMS)
def test_b3_selection(dev, monkeypatch, form, shape, kind):
    from mydetection_amd import ops
    c = dict(SEL_SHAPES[shape])
    Cout = c['cout'][FORMS[form]['cout']]
    pad, Ho, Wo = _geometry(c)
    x, w, expected = _selection(kind, c['B'], c['Cin'], Cout, c['k'], c['s'], c['H'], c['W'], pad)
    c.update(Cout=Cout, pad=pad, Ho=Ho, Wo=Wo)
    wd = w.permute(0, 2, 3, 1).contiguous().to(dev)
    d = dict(x=x.to(dev).contiguous(memory_format=torch.channels_last), w3=ops.split_bf16(wd), scale=None, shift=torch.zeros(Cout, device=dev),
             res=None, gate=None)
    with _form(monkeypatch, form):
        _plan(c, Cout, form)
        rc, y = _b3(c, d, ACT_NONE, False)
        torch.cuda.synchronize()
    assert rc == 0
    _selected(y, expected, f'{form} {shape} one-hot {"weights" if kind == "w" else "activations"}')


@pytest.mark.parametrize('kind', ('w', 'x'))
@pytest.mark.parametrize('Cout', (40, 136))
@pytest.mark.parametrize('geometry', P3_GEOMETRY)
def test_p3_selection(dev, geometry, Cout, kind):
    from mydetection_amd import ops
    s, H, W, strip = P3_GEOMETRY[geometry]
    x, w, expected = _selection(kind, 2, 32, Cout, 3, s, H, W, (1, 1, 1, 1))
    _p3_plan(expected.shape[2], expected.shape[3], Cout, s, strip)
    w3 = ops.split_bf16(w.permute(0, 2, 3, 1).contiguous().to(dev))
    y = ops.conv3x3_p3(x.to(dev).contiguous(memory_format=torch.channels_last), w3, None, torch.zeros(Cout, device=dev), s, ACT_NONE)
    torch.cuda.synchronize()
    assert y is not None
    _selected(y, expected, f'p3 {geometry} Cout {Cout} one-hot {"weights" if kind == "w" else "activations"}')


@pytest.mark.parametrize('form', FORMS)
def test_power_of_two_equivariance(dev, monkeypatch, form):
    """Activation channel c times 2^a_c and weight column c times 2^-a_c (a_c in [-12, 12]): every piece of every operand is scaled
    exactly, every product is the same number, so the output is the unscaled launch's bit for bit.  Dense data, leaky epilogue."""
    from mydetection_amd import ops
    shape = 'c_3x3_s2_asym_pad'
    Cout = _cout(shape, form)
    c = _base(shape, Cout)
    d = _device_args(c, dev)
    a = torch.randint(-12, 13, (c['Cin'],), generator=torch.Generator().manual_seed(12)).float().to(dev)
    xs = (d['x'] * torch.exp2(a).view(1, -1, 1, 1)).contiguous(memory_format=torch.channels_last)
    ws = (d['w'] * torch.exp2(-a).view(1, 1, 1, -1)).contiguous()
    assert torch.equal(xs * torch.exp2(-a).view(1, -1, 1, 1), d['x']) and not torch.equal(xs, d['x'])
    with _form(monkeypatch, form):
        _plan(c, Cout, form)
        rc, y = _b3(c, d, ACT_LEAKY, False)
        rc2, ys = _b3(c, d, ACT_LEAKY, False, x=xs, w3=ops.split_bf16(ws))
        torch.cuda.synchronize()
    assert rc == 0 and rc2 == 0
    assert torch.equal(y, ys), f'{form}: {int((y != ys).sum())} outputs change under a power-of-two rescaling of the channels'


# ------------------------------------------------------------------------------------------------------------------ what is reached

def test_reached_instances(dev, monkeypatch):
    """The table of kernel instances that the cases of this module reach, generated from the plan hooks, and the assertion that
    every instance launch_b3 / launch_b3w (with the fixup instances they call) and p3_dispatch can emit is in it."""
    from mydetection_amd import ops
    reached = set()

    def add(p, act, residual, gated):
        for split, n in ((0, p.main), (1, p.tail)):
            if n:
                reached.add((p.form, p.bm, p.bn, p.wn, act, int(residual), int(gated), split))

    for form in FORMS:
        with _form(monkeypatch, form):
            for shape in PLAIN + KCUT:
                if _cout(shape, form) is not None:
                    p = _plan(SHAPES[shape], _cout(shape, form), form)
                    for act, residual in EPILOGUES:
                        add(p, act, residual, False)
            if form in GATED_FORMS:
                for shape in GATE:
                    p = _plan(SHAPES[shape], _cout(shape, form), form)
                    for residual in (False, True):
                        add(p, ACT_NONE, residual, True)
    with _form(monkeypatch, 't64'):
        p = ops.b3_plan(7, 139, 140, 1024, 128, 1, cus=_cus())
        assert p.main and p.tail
        add(p, ACT_LEAKY, True, False)
    # what the dispatch code can emit: per form ACT 3 x RES 2, main launch and fixup; gated (ACT_NONE) RES 2 on the three 4-wave forms
    want = {FORMS[f]['tile'] + (act, int(r), 0, split) for f in FORMS for act, r in EPILOGUES for split in (0, 1)}
    want |= {FORMS[f]['tile'] + (ACT_NONE, r, 1, split) for f in GATED_FORMS for r in (0, 1) for split in (0, 1)}
    print('b3 instances reached: (form, BM, BN, WN, ACT, RES, GATE, split)')
    for t in sorted(reached):
        print('  b3', t)
    assert reached >= want, sorted(want - reached)
    assert reached == want, sorted(reached - want)

    p3 = set()
    for geometry, (s, H, W, strip) in P3_GEOMETRY.items():
        for Cout in (40, 136):
            p = _p3_plan((H - 1) // s + 1, (W - 1) // s + 1, Cout, s, strip)
            p3 |= {(s, p.bn, p.strip, act, int(r)) for act, r in P3_EPILOGUES}
    print('p3 instances reached: (S, BN, strip, ACT, RES)')
    for t in sorted(p3):
        print('  p3', t)
    want3 = {(s, bn, strip, act, r) for s, strips in ((1, (0,)), (2, (0, 1, 2))) for strip in strips for bn in (64, 128)
             for act in (ACT_NONE, ACT_LEAKY) for r in (0, 1)}
    assert len(want3) == 32 and p3 == want3, sorted(want3 ^ p3)


def test_tuning_is_back_at_default():
    from mydetection_amd import _lib
    assert _lib.lib().mydet_conv_b3_reload_tuning() == 0
