"""Footprints: every feature-map kernel writes only its own output view and reads only its own input views.

The layout contract (ops.nhwc_ld, the ldx / ldr / ldy arguments of include/mydet.h) makes a logical [B,C,H,W] tensor any 16-byte
aligned channel range of a [B,H,W,ld] buffer, and the models lean on it (BottleneckCSP's half-writes, the head towers that share one
pixel-major tensor, the 81-of-84 and 255-of-256 heads).  A store that is one float4, one ragged row or one K-cut fixup too wide
corrupts ANOTHER layer's data, and a load from beyond a slice that is multiplied by a zero weight is invisible until the neighbour
holds a NaN.  So every case here runs its launch with

  * inputs, residual and gate inside poisoned input arenas (tests/_arena.py: real data in the view, a NaN sentinel in every other
    word and in two guards of at least one image row / 4096 floats),
  * the output inside a poisoned output arena at a different channel offset and pixel stride, the view itself poison,
  * the shared split-K workspace (and the F(4x4) workspace) filled with the sentinel,

and asserts (1) the view is fully defined, finite and within the family's existing float64 tolerance (tests/test_gpu_kernels.py),
(2) nothing outside any view changed, (3) the view is bit-identical when every surrounding word and the workspaces hold zero instead
(same strides and offsets, hence the same kernel path: any difference means surroundings entered the arithmetic), (4) the intended
kernel ran: the ops.KernelTimer span of the family, whether the workspace was written (a K-cut / stream-K launch leaves partial
tiles there, an uncut one leaves it untouched), the `cut != plain` trick for the F(4x4) tail, the *_reload_tuning() codes.  The
tile form inside a family (128 x 128 / 128 x 64 / 64 x 64 x 32 / BN = 32, strip tiles, ...) is chosen by the launcher from the
shape; the shapes are those of the case lists in tests/test_gpu_kernels.py that name the form.

Entries whose `ops` wrapper allocates the output itself are called through _lib.lib() with ctypes exactly as `ops` does.

What cannot be proven from outside the library, a limit of these tests: the tile form INSIDE a family where the launcher publishes
no host-side rule -- the float32 implicit GEMM's 128 x 128 / 128 x 64 / 64 x 64 x 32 / BN = 32 tiles and its XCD-remapped grid, the
split-bf16 kernel's 64-row vs 128-row gated tiles.  Their cases take the shapes that the case lists of tests/test_gpu_kernels.py name
for the form, and assert what is observable: the family's span, and for EVERY case whether the launch left partial tiles in the
split-K workspace (`kcut`).  Where a host-side rule exists it is asserted: ops.b3_takes, ops.p3_plan (the launcher's own plan: tile count, strip form,
channel tile), ops.wino4_items and the launcher's own mydet_wino4_tail_plan.

Every entry of the issue's table takes foreign pointers and strides, so none is left out.  The share buffer of the in-launch
squeeze-excite tail (mydet_se_tail.hpart) is the kernels' own protocol state and is deliberately not poisoned; its launch counter is
checked instead.  mydet_conv2d_stem_f32, mydet_stem_dw_f32 and mydet_space_to_depth_f32 read the image through element strides, not
a channel slice: their input arena is a channels-last slice of a wider pixel.
"""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from _arena import SENTINEL_BITS, arena, flat_arena

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    from mydetection_amd import _lib
    _lib.lib()                                   # fail loudly if the HIP library is missing
    return torch.device('cuda:0')


def _fill_bits(t, fill):
    t.view(torch.int32).fill_(SENTINEL_BITS if fill == 'sentinel' else 0)


def _touched(t):
    return bool((t.view(torch.int32) != SENTINEL_BITS).any())


def _act(ref, act):
    if act == 1:
        return F.leaky_relu(ref, 0.1)
    if act == 2:
        return ref * torch.sigmoid(ref)
    return ref


def _conv_ref(dev, x, w, scale, shift, s, pad, act, res, gate):
    """float64 reference of the fused conv (x, w OIHW, ... on the CPU); large layers run the float64 ATen conv on the GPU."""
    B, Cin, H, W = x.shape
    where = dev if 2.0 * B * H * W * w.numel() / (s * s) > 4e9 else torch.device('cpu')
    xd = x.to(where).double()
    if gate is not None:
        xd = xd * gate.to(where).double().view(B, Cin, 1, 1)
    ref = F.conv2d(F.pad(xd, (pad[1], pad[3], pad[0], pad[2])), w.to(where).double(), None, s)
    if scale is not None:
        ref = ref * scale.to(where).double().view(1, -1, 1, 1)
    ref = _act(ref + shift.to(where).double().view(1, -1, 1, 1), act)
    if res is not None:
        ref = ref + res.to(where).double()
    return ref.cpu()


FAMILY_TOL = {'igemm': (2e-5, True), 'wino': (2e-5, True), 'wino4': (6e-5, True), 'b3': (2e-5, False), 'p3': (2e-5, False)}
FAMILY_SPAN = {'igemm': 'conv_igemm', 'wino': 'conv_wino', 'wino4': 'conv_wino4', 'b3': 'conv_igemm_b3', 'p3': 'conv_p3'}


def _conv_footprint(dev, fam, case):
    """One conv launch of family `fam` into an output arena, from input / residual / gate arenas; returns the view of the sentinel
    run.  case keys: B Cin Cout k s H W act kcut [residual gate bias_only pad ldy c0y]; kcut True / False: the launch must / must
    not leave partial tiles in the split-K workspace (a K-cut or stream-K launch + its fixup launch ran / did not run)."""
    from mydetection_amd import ops
    B, Cin, Cout, H, W = (case[n] for n in ('B', 'Cin', 'Cout', 'H', 'W'))
    k, s, act = case.get('k', 3), case.get('s', 1), case['act']
    pad = case.get('pad') or ((k - 1) // 2,) * 4
    g = torch.Generator().manual_seed(7 * Cin + Cout + k + s)
    x = torch.randn(B, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, k, k, generator=g) / (Cin * k * k) ** 0.5
    scale = None if case.get('bias_only') else torch.rand(Cout, generator=g) + 0.5
    shift = torch.randn(Cout, generator=g) * 0.1
    gate = torch.rand(B, Cin, generator=g) if case.get('gate') else None
    Ho, Wo = ops.conv_out_size(H, k, s, pad[0], pad[2]), ops.conv_out_size(W, k, s, pad[1], pad[3])
    res = torch.randn(B, Cout, Ho, Wo, generator=g) if case.get('residual') else None
    ref = _conv_ref(dev, x, w, scale, shift, s, pad, act, res, gate)
    assert tuple(ref.shape) == (B, Cout, Ho, Wo)
    wd = w.permute(0, 2, 3, 1).contiguous().to(dev)
    sc_d, sh_d = (scale.to(dev) if scale is not None else None), shift.to(dev)
    u = ops.wino_weights(wd) if fam == 'wino' else None
    u4 = ops.wino4_weights(wd) if fam == 'wino4' else None
    w3 = ops.split_bf16(wd) if fam in ('b3', 'p3') else None
    assert (fam != 'wino' or u is not None) and (fam != 'wino4' or u4 is not None) and (fam not in ('b3', 'p3') or w3 is not None)
    if fam == 'b3':
        assert ops.b3_takes(B * Ho * Wo, Cin, Cout, k, min_rows=1, min_cout=64)
    if fam == 'wino4':
        assert ops.WINOGRAD and ops.WINOGRAD4
    c0y = case.get('c0y', 12)
    ldy = case.get('ldy', (Cout + 3) // 4 * 4 + c0y + 16)
    ws = ops.conv_workspace(dev)
    ws4 = ops.wino4_workspace(dev, _lib_i64('mydet_wino4_workspace_bytes', B, H, W, Cin, Cout)) if fam == 'wino4' else None

    def run(fill):
        xin, cx = arena(B, Cin, H, W, Cin + 24, 8, dev, fill, data=x.to(dev))
        assert ops.nhwc_ld(xin) == Cin + 24
        checks = [('input', cx)]
        rin = gin = None
        if res is not None:
            rin, cr = arena(B, Cout, Ho, Wo, (Cout + 3) // 4 * 4 + 12, 4, dev, fill, data=res.to(dev))
            checks.append(('residual', cr))
        if gate is not None:
            gin, cg = flat_arena(B * Cin, dev, fill, data=gate.to(dev))
            gin = gin.view(B, Cin)
            checks.append(('gate', cg))
        out, co = arena(B, Cout, Ho, Wo, ldy, c0y, dev, fill)
        assert ops.nhwc_ld(out) == ldy
        _fill_bits(ws, fill)
        if ws4 is not None:
            _fill_bits(ws4, fill)
        ops.TIMER = ops.KernelTimer()
        p3_was = ops.CONV_P3
        try:
            if fam == 'p3':
                y = ops.conv3x3_p3(xin, w3, sc_d, sh_d, s, act, residual=rin, out=out, cout=Cout)
            else:
                ops.CONV_P3 = False
                y = ops.conv2d(xin, wd, sc_d, sh_d, k, s, pad, act, residual=rin, out=out, gate=gin, wino=u, wino4=u4, b3=w3,
                               b3_min_rows=1 if fam == 'b3' else None)
        finally:
            timer, ops.TIMER = ops.TIMER, None
            ops.CONV_P3 = p3_was
        torch.cuda.synchronize()
        assert y is not None and y.data_ptr() == out.data_ptr()
        assert set(timer.spans) == {FAMILY_SPAN[fam]}, (fam, sorted(timer.spans))
        co.view_defined(f'{fam} output ({fill})')
        co.outside_untouched(f'{fam} output ({fill})')
        for name, c in checks:
            c.outside_untouched(f'{fam} {name} ({fill})')
            c.view_defined(f'{fam} {name} ({fill})')
        assert torch.equal(xin, x.to(dev)) and (rin is None or torch.equal(rin, res.to(dev))), 'an input view was written'
        return out.clone(), (_touched(ws) if fill == 'sentinel' else None)

    y, ws_written = run('sentinel')
    rel, floor1 = FAMILY_TOL[fam]
    m = ref.abs().max().item()
    tol = rel * (max(1.0, m) if floor1 else m)
    err = (y.cpu().double() - ref).abs().max().item()
    print(f'{fam} {case}: err {err:.3e} tol {tol:.3e} workspace written {ws_written}')
    assert err <= tol, f'{fam} {case}: {err:.2e} > {tol:.2e}'
    if fam != 'wino4':              # (F(4x4) keeps its partial tiles in its own workspace: test_footprint_conv_winograd4 proves its tail)
        assert ws_written == case['kcut'], f'{fam} {case}: split-K workspace written = {ws_written}, the case expects {case["kcut"]}'
    y0, _ = run('zero')
    assert torch.equal(y, y0), (f'{fam} {case}: {int((y != y0).sum())} output value(s) depend on what surrounds the views or on stale '
                                'workspace contents')
    return y


def _lib_i64(name, *args):
    from mydetection_amd import _lib
    return int(getattr(_lib.lib(), name)(*args))


# ---------------------------------------------------------------------------------------------------- float32 implicit GEMM
@pytest.mark.parametrize('case', [
    dict(B=2, Cin=128, Cout=256, k=3, s=1, H=20, W=20, act=1, residual=True, kcut=True),                   # 128 x 128 / 128 x 64 tiles, residual from a slice
    dict(B=2, Cin=32, Cout=64, k=3, s=2, H=32, W=32, act=1, kcut=True),                                    # 64 x 64 x 32 tile, stride 2
    dict(B=2, Cin=64, Cout=32, k=1, s=1, H=16, W=24, act=1, kcut=False),                                    # BN = 32 tile
    dict(B=2, Cin=24, Cout=144, k=1, s=1, H=12, W=12, act=2, kcut=False),                                   # generic K (Cin % 32 != 0)
    dict(B=1, Cin=88, Cout=88, k=3, s=1, H=10, W=10, act=0, bias_only=True, kcut=True),                    # generic K, 3x3
    dict(B=3, Cin=256, Cout=255, k=1, s=1, H=13, W=11, act=0, bias_only=True, c0y=0, ldy=256, kcut=False),  # ragged M and N: 255 of ld 256
    dict(B=3, Cin=256, Cout=255, k=1, s=1, H=13, W=11, act=0, bias_only=True, c0y=12, ldy=272, kcut=False), # ... and inside a wider buffer
    dict(B=1, Cin=768, Cout=256, k=1, s=1, H=8, W=8, act=1, kcut=True),                         # small grid: split K + conv_fixup_kernel
    dict(B=1, Cin=512, Cout=252, k=3, s=1, H=10, W=10, act=1, residual=True, kcut=True),        # ... ragged N, residual in the fixup
    dict(B=32, Cin=64, Cout=128, k=3, s=2, H=64, W=64, act=1, kcut=False),                      # big grid (XCD remap), whole rounds
    dict(B=2, Cin=96, Cout=64, k=1, s=1, H=33, W=31, act=0, gate=True, residual=True, kcut=False),          # SE gate on A
    dict(B=1, Cin=32, Cout=32, k=3, s=2, H=16, W=16, act=2, pad=(0, 0, 1, 1), kcut=False),                  # static-SAME asymmetric pad
])
def test_footprint_conv_igemm(dev, case):
    _conv_footprint(dev, 'igemm', case)


@pytest.mark.parametrize('Cin,Cout,H,W,gated,res,act', [(240, 40, 181, 183, True, True, 0), (96, 24, 192, 176, True, False, 0),
                                                       (144, 40, 181, 183, True, True, 0), (32, 44, 192, 176, False, True, 2)])
def test_footprint_pointwise_skinny(dev, monkeypatch, Cin, Cout, H, W, gated, res, act):
    """mydet_pw_skinny (csrc/pointwise.hip) behind mydet_conv2d_igemm_f32, under the launcher's DEFAULT routing (Cout <= 48, Cin in
    {16, 32, 96, 144, 240}, >= 65 536 pixels; no MYDET_PW_WIDE): shapes of test_pointwise_skinny; that the skinny kernel ran shows as
    a different summation order from the tiled kernel (MYDET_PW_SKINNY=0), as there."""
    from mydetection_amd import ops
    case = dict(B=2, Cin=Cin, Cout=Cout, k=1, s=1, H=H, W=W, act=act, gate=gated, residual=res, kcut=False)
    y = _conv_footprint(dev, 'igemm', case)
    monkeypatch.setenv('MYDET_PW_SKINNY', '0')
    try:
        y_tiled = _conv_footprint(dev, 'igemm', case)
    finally:
        monkeypatch.delenv('MYDET_PW_SKINNY')
    assert not torch.equal(y_tiled, y), 'the skinny kernel did not take a shape chosen for it'
    assert (y_tiled - y).abs().max().item() <= 4e-5 * max(1.0, y.abs().max().item())
    assert ops.nhwc_ld(y) is not None


# ---------------------------------------------------------------------------------------------------- split-bf16 implicit GEMM
@pytest.mark.parametrize('case', [
    dict(B=16, Cin=256, Cout=128, k=1, s=1, H=40, W=40, act=1, residual=True, kcut=False),                          # default form, 200 tiles
    dict(B=12, Cin=64, Cout=160, k=3, s=2, H=64, W=64, act=1, kcut=False),                                          # 3x3 stride 2, ragged channel tile
    dict(B=9, Cin=512, Cout=255, k=1, s=1, H=31, W=33, act=0, bias_only=True, kcut=False),                          # ragged rows and channels (255)
    dict(B=12, Cin=256, Cout=320, k=1, s=1, H=27, W=29, act=2, form='wide', kcut=False),                            # wide form, quarter-full channel tile
    dict(B=9, Cin=512, Cout=255, k=1, s=1, H=31, W=33, act=0, bias_only=True, form='waves8', kcut=False),           # 8-wave workgroups
    dict(B=16, Cin=1152, Cout=192, k=1, s=1, H=20, W=20, act=0, residual=True, gate=True, kcut=False),  # MBConv project conv: gate, small grid in 64-row tiles
    dict(B=22, Cin=1024, Cout=512, k=1, s=1, H=40, W=40, act=1, residual=True, kcut=True),              # 275 x 4 tiles = two rounds of 512 + 76 cut along K + fixup
    dict(B=8, Cin=40, Cout=240, k=1, s=1, H=80, W=80, act=2, kcut=False),                                           # Cin % 16 == 8: zero-filled last slab
    dict(B=4, Cin=24, Cout=144, k=1, s=1, H=50, W=46, act=2, kcut=False),                                           # Cin % 16 == 8 again
    dict(B=5, Cin=96, Cout=64, k=1, s=1, H=33, W=31, act=0, gate=True, kcut=False),                                 # gated 64-row tile
    dict(B=40, Cin=672, Cout=112, k=1, s=1, H=40, W=40, act=0, residual=True, gate=True, kcut=False),               # gated 128-row tile (500 tiles)
])
def test_footprint_conv_split_bf16(dev, case, monkeypatch):
    from mydetection_amd import _lib
    case = dict(case)
    form = case.pop('form', None)
    if form:
        monkeypatch.setenv('MYDET_B3_WIDE' if form == 'wide' else 'MYDET_B3_WAVES', '1' if form == 'wide' else '8')
    try:
        assert _lib.lib().mydet_conv_b3_reload_tuning() == {None: 0, 'wide': 1, 'waves8': 2}[form]
        _conv_footprint(dev, 'b3', case)
    finally:
        monkeypatch.undo()
        assert _lib.lib().mydet_conv_b3_reload_tuning() == 0


# ---------------------------------------------------------------------------------------------------- patch-resident 3x3
@pytest.mark.parametrize('case', [
    dict(B=4, Cin=32, Cout=64, s=2, H=64, W=64, act=1, kcut=False, bn=64, strip=None, tiles=8),                          # stride 2, BN = 64, whole tiles
    dict(B=3, Cin=64, Cout=128, s=2, H=80, W=80, act=1, kcut=False, bn=128, strip='16x8', tiles=13),                         # BN = 128; 40 x 40 outputs: 16 x 8 strip tiles
    dict(B=3, Cin=32, Cout=192, s=2, H=40, W=40, act=1, residual=True, kcut=False, bn=128, strip='32x4', tiles=4),          # 20 x 20 outputs: 32 x 4 strip tile, ragged channels
    dict(B=2, Cin=32, Cout=64, s=1, H=48, W=64, act=1, residual=True, kcut=False, bn=64, strip=None, tiles=24),           # stride 1, BN = 64
    dict(B=2, Cin=64, Cout=160, s=1, H=21, W=35, act=1, kcut=False, bn=128, strip=None, tiles=9),                         # stride 1, BN = 128, ragged column and rows
    dict(B=5, Cin=16, Cout=40, s=2, H=30, W=18, act=1, residual=True, kcut=False, bn=64, strip=None, tiles=2),           # ragged channels (40 of 64), ragged column
    dict(B=2, Cin=16, Cout=40, s=2, H=70, W=8, act=1, kcut=False, bn=64, strip='32x4', tiles=2),                           # 4 columns only: 32 x 4 strips over 35 rows
])
def test_footprint_conv_p3(dev, case):
    """bn / strip / tiles: the channel tile (128 from 65 output channels up), the strip form of the remainder columns and the 128-pixel tiles
    per image the shape is meant to reach, asserted against the launcher's own plan (mydet_conv3x3_p3_plan through ops.p3_plan: 8 x 16
    tiles; at stride 2 a remainder of 8 / 4 columns as 16 x 8 / 32 x 4 strip tiles), which is also what ops.p3_tiles returns."""
    from mydetection_amd import ops
    case = dict(case, k=3)
    bn, strip, tiles = case.pop('bn'), case.pop('strip'), case.pop('tiles')
    Ho, Wo = (case['H'] - 1) // case['s'] + 1, (case['W'] - 1) // case['s'] + 1
    plan = ops.p3_plan(Ho, Wo, case['Cout'], case['s'])
    assert (plan.bn, plan.strip, plan.tiles_img) == (bn, {None: 0, '16x8': 1, '32x4': 2}[strip], tiles)
    assert ops.p3_tiles(Ho, Wo, case['s']) == tiles
    _conv_footprint(dev, 'p3', case)


# ---------------------------------------------------------------------------------------------------- Winograd F(2x2,3x3)
# plan = (NW, stream-K schedule, items, whole items per workgroup, items cut along K) of the launch on the 256 CUs of the MI355X: what the
# comments say, asserted through the launcher's own mydet_wino_plan; its fixup flag must be the case's `kcut`
@pytest.mark.parametrize('case', [
    dict(B=1, Cin=32, Cout=64, H=16, W=16, act=1, residual=True, kcut=False, plan=(4, 0, 2, 1, 0)),      # whole tiles
    dict(B=3, Cin=64, Cout=128, H=13, W=11, act=1, kcut=False, plan=(4, 0, 8, 1, 0)),                    # odd H and W
    dict(B=1, Cin=88, Cout=88, H=10, W=10, act=0, bias_only=True, kcut=False, plan=(4, 0, 2, 1, 0)),     # Cout % 64 != 0 (zero-padded U rows)
    dict(B=2, Cin=88, Cout=84, H=5, W=5, act=2, kcut=False, plan=(4, 0, 2, 1, 0)),                       # ragged everything
    dict(B=16, Cin=64, Cout=128, H=80, W=80, act=1, kcut=False, plan=(4, 0, 1600, 1, 0)),     # big grid of the 32-tile shape: plain rounds
    dict(B=32, Cin=128, Cout=256, H=40, W=40, act=1, residual=True, kcut=True,    # 64-tile shape, 3.125 items per workgroup: stream-K + conv_wino_fixup_kernel
         plan=(8, 1, 800, 3, 32)),
    dict(B=1, Cin=128, Cout=128, H=8, W=8, act=1, residual=True, kcut=True, plan=(8, 1, 2, 0, 2)),       # small grid cut along K
    dict(B=2, Cin=256, Cout=192, H=6, W=7, act=0, bias_only=True, kcut=True, plan=(8, 1, 3, 0, 3)),      # small, ragged, cut along K
])
def test_footprint_conv_winograd(dev, case):
    from mydetection_amd import _lib, ops
    case = dict(case, k=3, s=1)
    out = (ctypes.c_int32 * 10)()
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    _lib.check(_lib.lib().mydet_wino_plan(case['B'], case['H'], case['W'], case['Cin'], case['Cout'], ops.WORKSPACE_BYTES, cus, out), 'mydet_wino_plan')
    assert (out[0], out[1], out[2], out[5], out[6]) == case.pop('plan') and bool(out[9]) == case['kcut'], (case, list(out))
    _conv_footprint(dev, 'wino', case)


# ---------------------------------------------------------------------------------------------------- Winograd F(4x4,3x3)
@pytest.mark.parametrize('case', [
    dict(B=3, Cin=64, Cout=128, H=13, W=11, act=1, kcut=False, items=8),                      # odd H and W: partial tiles
    dict(B=2, Cin=132, Cout=84, H=5, W=7, act=2, residual=True, kcut=False, items=3),                  # Cin % 8 != 0, ragged everything
    dict(B=1, Cin=256, Cout=512, H=32, W=32, act=1, residual=True, kcut=False, items=32),               # batch 1
    dict(B=32, Cin=256, Cout=512, H=40, W=40, act=1, residual=True, kcut=True, items=1600),   # the headline's 40^2 layers: 1536 items + 64 cut 8 ways
    dict(B=32, Cin=512, Cout=1024, H=20, W=20, act=1, residual=True, kcut=True, items=800),  # the headline's 20^2 layers: tail groups cut 2 and 8 ways
])
def test_footprint_conv_winograd4(dev, case, monkeypatch):
    """items: the launch's workgroups (ops.wino4_items); kcut: whether the launcher's own tail plan (mydet_wino4_tail_plan on this
    chip's 2 workgroups per CU) cuts a remainder along K -- asserted, and for the cut shapes shown again by cut != plain."""
    from mydetection_amd import _lib, ops
    case = dict(case, k=3, s=1)
    assert ops.wino4_items(case['B'], case['H'], case['W'], case['Cout']) == case.pop('items')
    plan = (ctypes.c_int32 * 17)()
    slots = 2 * torch.cuda.get_device_properties(dev).multi_processor_count
    groups = _lib.lib().mydet_wino4_tail_plan(case['B'], case['H'], case['W'], case['Cin'], case['Cout'], slots, ctypes.cast(plan, ctypes.c_void_p))
    assert (groups > 0) == case['kcut'], (groups, list(plan))
    cut = _conv_footprint(dev, 'wino4', case)
    if case.get('kcut'):                        # the tail rule triggered: the uncut form sums in another association
        monkeypatch.setenv('MYDET_W4_TAIL', '0')
        _lib.lib().mydet_wino4_reload_tuning()
        try:
            plain = _conv_footprint(dev, 'wino4', case)
        finally:
            monkeypatch.delenv('MYDET_W4_TAIL')
            _lib.lib().mydet_wino4_reload_tuning()
        assert not torch.equal(cut, plain), 'the tail rule did not trigger on a shape chosen to trigger it'
        assert (cut - plain).abs().max().item() <= 2e-5 * max(1.0, plain.abs().max().item())


# ---------------------------------------------------------------------------------------------------- fused upsample-concat 1x1
@pytest.mark.parametrize('shape,kcut', [((32, 128, 256, 128, 40, 40), False),     # the headline's layer: big grid
                                        ((1, 256, 512, 256, 10, 10), True),       # batch 1: 7 x 4 tiles cut along K
                                        ((3, 64, 32, 252, 6, 10), False)])        # ragged rows and channels, 3 K steps: uncut
def test_footprint_conv1x1_upcat(dev, shape, kcut):
    from mydetection_amd import _lib, ops
    B, C1, C2, Cout, Ha, Wa = shape
    H, W = 2 * Ha, 2 * Wa
    g = torch.Generator().manual_seed(21)
    lo, hi = torch.randn(B, C1, Ha, Wa, generator=g), torch.randn(B, C2, H, W, generator=g)
    w = torch.randn(Cout, C1 + C2, generator=g) / (C1 + C2) ** 0.5
    sc, sh = torch.rand(Cout, generator=g) + 0.5, torch.randn(Cout, generator=g)
    ref = F.leaky_relu(torch.einsum('bchw,oc->bohw', torch.cat((F.interpolate(lo.double(), scale_factor=2, mode='nearest'), hi.double()), 1),
                                    w.double()) * sc.double().view(1, -1, 1, 1) + sh.double().view(1, -1, 1, 1), 0.1)
    wd, scd, shd = w.view(Cout, 1, 1, -1).contiguous().to(dev), sc.to(dev), sh.to(dev)
    ws = ops.conv_workspace(dev)

    def run(fill):
        a, ca = arena(B, C1, Ha, Wa, C1 + 16, 8, dev, fill, data=lo.to(dev))
        b, cb = arena(B, C2, H, W, C2 + 40, 20, dev, fill, data=hi.to(dev))
        out, co = arena(B, Cout, H, W, Cout + 24, 4, dev, fill)
        _fill_bits(ws, fill)
        code = _lib.lib().mydet_conv1x1_upcat_f32(ops._ptr(a), ops.nhwc_ld(a), C1, ops._ptr(b), ops.nhwc_ld(b), C2, ops._ptr(wd), ops._ptr(scd),
                                                  ops._ptr(shd), ops._ptr(ws), ws.numel() * 4, ops._ptr(out), ops.nhwc_ld(out), B, H, W, Cout,
                                                  ops.ACT_LEAKY, ops._stream())
        assert code == 0, f'mydet_conv1x1_upcat_f32 returned {code}: the fused launch did not take a shape chosen for it'
        torch.cuda.synchronize()
        co.view_defined('upcat output')
        for c in (co, ca, cb):
            c.outside_untouched(f'upcat ({fill})')
        assert torch.equal(a, lo.to(dev)) and torch.equal(b, hi.to(dev))
        return out.clone(), _touched(ws)

    y, written = run('sentinel')
    assert (y.cpu().double() - ref).abs().max().item() <= 2e-5 * ref.abs().max().item()
    assert written == kcut
    assert torch.equal(run('zero')[0], y)
    cat = ops.upsample_concat(lo.to(dev), (H, W), hi.to(dev))                                    # bit-identical to the two launches
    assert torch.equal(ops.conv2d(cat, wd, scd, shd, 1, 1, (0, 0, 0, 0), ops.ACT_LEAKY), y)


# ---------------------------------------------------------------------------------------------------- pyramid nodes
def test_footprint_sepconv_nodes(dev):
    """One node, and a 10-node launch (five levels x two towers, as EfDetHead._towers issues) whose outputs are ADJACENT channel ranges of
    one buffer per level; fused inputs (UP2X / POOL at odd-row edges) come from slices."""
    from mydetection_amd import ops
    from _refs import sepconv_node_f64 as _sepconv_ref
    g = torch.Generator().manual_seed(23)
    C, B = 88, 2

    def node(hw, cout, act, bn, modes):
        H, W = hw
        shapes = {0: (H, W), 1: (H // 2, W // 2), 2: (H * 2, W * 2)}
        n_in = len(modes)
        return dict(hw=hw, inputs=[torch.randn(B, C, *shapes[m], generator=g) for m in modes], modes=modes,
                    fuse_w=torch.tensor([0.8, 1.3, -0.4][:n_in]) if n_in > 1 else None,
                    w_dw=torch.randn(3, 3, C, generator=g) / 3.0, w_pw=torch.randn(cout, C, generator=g) / C ** 0.5,
                    scale=torch.rand(cout, generator=g) + 0.5 if bn else None, shift=torch.randn(cout, generator=g) * 0.2, cout=cout, act=act)

    sizes = [(20, 20), (10, 10), (5, 5), (3, 3), (13, 7)]
    groups = [
        ([node((13, 7), 36, 0, False, [0])], None),                                                     # one node, Cout 36 of a wider row
        ([node((10, 10), 88, 0, True, [0, 1]), node((5, 5), 88, 0, True, [0, 0, 2]), node((10, 6), 88, 2, True, [0, 2])], None),
        ([node(hw, 88, 2, True, [0]) for hw in sizes] + [node(hw, 88, 2, True, [0]) for hw in sizes], 5),  # 10 nodes, adjacent ranges
    ]
    for grp, shared in groups:
        def run(fill):
            checks, outs_chk, dev_nodes = [], [], []
            bufs = {}
            for i, nd in enumerate(grp):
                ins = []
                for j, t in enumerate(nd['inputs']):
                    v, c = arena(B, C, t.shape[2], t.shape[3], C + 8 + 4 * j, 4 + 4 * j, dev, fill, data=t.to(dev))
                    ins.append(v)
                    checks.append(c)
                H, W = nd['hw']
                if shared:                       # node i and node i + shared write channels [4, 92) and [92, 180) of ONE [B,H,W,184] buffer
                    lvl, half = i % shared, i // shared
                    if lvl not in bufs:
                        bufs[lvl] = arena(B, 2 * 88, H, W, 184, 4, dev, fill)
                        outs_chk.append(bufs[lvl][1])
                    out = bufs[lvl][0][:, half * 88:(half + 1) * 88]
                else:
                    out, c = arena(B, nd['cout'], H, W, nd['cout'] + 20, 8, dev, fill)
                    outs_chk.append(c)
                assert ops.nhwc_ld(out) is not None
                dev_nodes.append(dict(inputs=ins, modes=nd['modes'], fuse_weights=nd['fuse_w'].to(dev) if nd['fuse_w'] is not None else None,
                                      w_dw=nd['w_dw'].to(dev), w_pw=ops.pack_pointwise(nd['w_pw'].to(dev)),
                                      scale=nd['scale'].to(dev) if nd['scale'] is not None else None, shift=nd['shift'].to(dev),
                                      cout=nd['cout'], act=nd['act'], out=out))
            ops.TIMER = ops.KernelTimer()
            try:
                outs = ops.sepconv_nodes(dev_nodes)
            finally:
                timer, ops.TIMER = ops.TIMER, None
            torch.cuda.synchronize()
            assert list(timer.spans) == ['sepconv_nodes'] and len(timer.spans['sepconv_nodes']) == 1        # ONE launch
            for c in outs_chk:
                c.view_defined(f'sepconv output ({fill})')
                c.outside_untouched(f'sepconv output ({fill})')
            for c in checks:
                c.outside_untouched(f'sepconv input ({fill})')
            return [o.clone() for o in outs]

        ys = run('sentinel')
        for nd, y in zip(grp, ys):
            ref = _sepconv_ref(nd['inputs'], nd['modes'], nd['fuse_w'], nd['w_dw'], nd['w_pw'], nd['scale'], nd['shift'], nd['act'])
            err = (y.cpu().double() - ref).abs().max().item()
            assert err <= 2e-5 * max(1.0, ref.abs().max().item()), (nd['cout'], nd['modes'], err)
        for y, y0 in zip(ys, run('zero')):
            assert torch.equal(y, y0)


def test_footprint_bifpn_fuse_inputs(dev):
    """mydet_bifpn_fuse_f32 with every input a slice and the output an arena (ctypes: ops.bifpn_fuse allocates its output): UP2X and
    POOL reads at the last odd row / column must stay inside their maps."""
    from mydetection_amd import _lib, ops
    g = torch.Generator().manual_seed(29)
    B, C = 2, 88
    swish = lambda t: t * torch.sigmoid(t)                           # noqa: E731
    for (H, W), modes, wts in (((10, 6), [0, 1], [0.7, 1.2]), ((5, 7), [0, 0, 2], [0.9, 0.4, 1.3]), ((7, 5), [0, 2], [-0.5, 1.0])):
        shapes = {0: (H, W), 1: (H // 2, W // 2), 2: (H * 2, W * 2)}
        if 1 in modes:
            assert H % 2 == 0 and W % 2 == 0
        ins = [torch.randn(B, C, *shapes[m], generator=g) for m in modes]
        wt = torch.tensor(wts)
        wn = F.relu(wt)
        wn = wn / (wn.sum() + 0.0001)
        pre = [t if m == 0 else (F.interpolate(t, scale_factor=(2, 2), mode='nearest') if m == 1 else F.max_pool2d(t, 3, 2, 1)) for t, m in zip(ins, modes)]
        ref = swish(sum(wi * f for wi, f in zip(wn, pre)))
        wtd = wt.to(dev)

        def run(fill):
            views, chks = zip(*[arena(B, C, t.shape[2], t.shape[3], C + 12, 8, dev, fill, data=t.to(dev)) for t in ins])
            out, co = arena(B, C, H, W, C + 20, 12, dev, fill)
            args = []
            for i in range(3):
                args += [ops._ptr(views[i]), ops.nhwc_ld(views[i]), modes[i]] if i < len(ins) else [ctypes.c_void_p(0), 0, 0]
            _lib.check(_lib.lib().mydet_bifpn_fuse_f32(len(ins), *args, ops._ptr(wtd), ops._ptr(out), ops.nhwc_ld(out), B, H, W, C, ops._stream()),
                       'mydet_bifpn_fuse_f32')
            torch.cuda.synchronize()
            co.view_defined('bifpn_fuse output')
            for c in (co,) + chks:
                c.outside_untouched(f'bifpn_fuse {modes} ({fill})')
            return out.clone()
        y = run('sentinel')
        torch.testing.assert_close(y.cpu(), ref, rtol=2e-6, atol=1e-7)
        assert torch.equal(run('zero'), y)


# ---------------------------------------------------------------------------------------------------- depthwise
@pytest.mark.parametrize('k,s,pad,C,H,W,act', [(3, 1, (1, 1, 1, 1), 32, 20, 24, 2), (3, 2, (0, 0, 1, 1), 96, 16, 16, 2),
                                              (5, 1, (2, 2, 2, 2), 144, 12, 10, 2), (5, 2, (1, 1, 2, 2), 240, 10, 10, 2),
                                              (3, 1, (1, 1, 1, 1), 88, 5, 5, 0), (3, 1, (1, 1, 1, 1), 16, 41, 70, 2),
                                              (3, 1, (1, 1, 1, 1), 8, 12, 16, 2)])      # under 16 channels: the two-row register-blocked form
@pytest.mark.parametrize('squeeze', [False, True])
def test_footprint_dwconv(dev, k, s, pad, C, H, W, act, squeeze):
    """mydet_dwconv_f32 through ctypes (ops.dwconv allocates y): y an arena, and with squeeze the partial-sum buffer [B,S+1,C] too
    (slices 0..S-1 are the launch's to define; slice S is scratch for mydet_se_gate_f32 and must stay untouched here)."""
    from mydetection_amd import _lib, ops
    g = torch.Generator().manual_seed(3)
    B = 2
    x = torch.randn(B, C, H, W, generator=g)
    w = torch.randn(C, 1, k, k, generator=g) * 0.3
    bn = act != 0
    scale = torch.rand(C, generator=g) + 0.5 if bn else None
    shift = torch.randn(C, generator=g) * 0.1 if bn else None
    ref = F.conv2d(F.pad(x, (pad[1], pad[3], pad[0], pad[2])).double(), w.double(), None, s, 0, 1, C)
    if bn:
        ref = ref * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1)
    ref = _act(ref, act)
    Ho, Wo = ref.shape[2:]
    wd = w.permute(2, 3, 0, 1).reshape(k, k, C).contiguous().to(dev)
    scd, shd = (scale.to(dev) if bn else None), (shift.to(dev) if bn else None)
    S = _lib.lib().mydet_dwconv_slices(Ho, Wo, C, k, s) if squeeze else 0
    assert not squeeze or S >= 1

    def run(fill):
        xin, cx = arena(B, C, H, W, C + 16, 4, dev, fill, data=x.to(dev))
        out, co = arena(B, C, Ho, Wo, C + 24, 16, dev, fill)
        part = cp = None
        if squeeze:             # [B][S+1][C] as a [B, S*C of (S+1)*C, 1, 1] map: the view is slices 0..S-1 of every image
            part, cp = arena(B, S * C, 1, 1, (S + 1) * C, 0, dev, fill)
        _lib.check(_lib.lib().mydet_dwconv_f32(ops._ptr(xin), ops.nhwc_ld(xin), ops._ptr(wd), ops._ptr(scd), ops._ptr(shd), ops._ptr(out),
                                               ops.nhwc_ld(out), B, H, W, C, k, s, pad[0], pad[1], Ho, Wo, act, ops._ptr(part), S, None,
                                               ops._stream()), 'mydet_dwconv_f32')
        torch.cuda.synchronize()
        co.view_defined('dwconv output')
        co.outside_untouched(f'dwconv output ({fill})')
        cx.outside_untouched(f'dwconv input ({fill})')
        sums = None
        if squeeze:
            cp.view_defined('dwconv squeeze sums')
            cp.outside_untouched(f'dwconv squeeze sums ({fill})')
            sums = part.reshape(B, S, C).sum(1)
        return out.clone(), sums

    y, sums = run('sentinel')
    assert (y.cpu().double() - ref).abs().max() < 2e-5
    if squeeze:
        torch.testing.assert_close(sums.cpu().double(), ref.sum(dim=(2, 3)), rtol=1e-5, atol=1e-4)
    y0, sums0 = run('zero')
    assert torch.equal(y, y0) and (sums is None or torch.equal(sums, sums0))


# ---------------------------------------------------------------------------------------------------- data movement
def test_footprint_data_movement(dev):
    """upsample_concat, spp_concat, space_to_depth, maxpool3s2 (ctypes: outputs are arenas, inputs slices) and channel_sums (input a
    slice, the partial-sum buffer an arena): pure data movement / max stays torch.equal."""
    from mydetection_amd import _lib, ops
    L = _lib.lib()
    g = torch.Generator().manual_seed(31)
    for fill in ('sentinel', 'zero'):
        # nearest upsample + concat, odd target size
        a, b = torch.randn(2, 8, 5, 7, generator=g), torch.randn(2, 12, 10, 14, generator=g)
        av, ca = arena(2, 8, 5, 7, 24, 8, dev, fill, data=a.to(dev))
        bv, cb = arena(2, 12, 10, 14, 20, 4, dev, fill, data=b.to(dev))
        out, co = arena(2, 20, 10, 14, 36, 12, dev, fill)
        _lib.check(L.mydet_upsample_concat_f32(ops._ptr(av), 24, 5, 7, 8, ops._ptr(bv), 20, 12, ops._ptr(out), 36, 2, 10, 14, ops._stream()), 'upsample_concat')
        torch.cuda.synchronize()
        assert torch.equal(out.cpu(), torch.cat((F.interpolate(a, size=(10, 14), mode='nearest'), b), 1))
        for c in (co, ca, cb):
            c.outside_untouched(f'upsample_concat ({fill})')
        out, co = arena(2, 8, 9, 13, 16, 4, dev, fill)                                            # non-integer scale, no concat
        _lib.check(L.mydet_upsample_concat_f32(ops._ptr(av), 24, 5, 7, 8, None, 0, 0, ops._ptr(out), 16, 2, 9, 13, ops._stream()), 'upsample')
        torch.cuda.synchronize()
        assert torch.equal(out.cpu(), F.interpolate(a, size=(9, 13), mode='nearest'))
        co.outside_untouched(f'upsample ({fill})')
        ca.outside_untouched(f'upsample input ({fill})')
        # SPP
        for hw in ((8, 8), (5, 13)):
            t = torch.randn(2, 16, *hw, generator=g)
            tv, ct = arena(2, 16, *hw, 28, 8, dev, fill, data=t.to(dev))
            out, co = arena(2, 64, *hw, 84, 12, dev, fill)
            _lib.check(L.mydet_spp_concat_f32(ops._ptr(tv), 28, ops._ptr(out), 84, 2, hw[0], hw[1], 16, 5, 9, 13, ops._stream()), 'spp_concat')
            torch.cuda.synchronize()
            assert torch.equal(out.cpu(), torch.cat([t] + [F.max_pool2d(t, k, 1, k // 2) for k in (5, 9, 13)], 1)), hw
            co.outside_untouched(f'spp_concat ({fill})')
            ct.outside_untouched(f'spp_concat input ({fill})')
        # space-to-depth: the image read through element strides (channels-last slice of a wider buffer)
        x = torch.randn(2, 3, 12, 20, generator=g)
        xv, cx = arena(2, 3, 12, 20, 8, 4, dev, fill, data=x.to(dev))
        out, co = arena(2, 12, 6, 10, 24, 8, dev, fill)
        sb, sc_, sh_, sw = xv.stride()
        _lib.check(L.mydet_space_to_depth_f32(ops._ptr(xv), sb, sc_, sh_, sw, ops._ptr(out), 24, 2, 3, 12, 20, ops._stream()), 'space_to_depth')
        torch.cuda.synchronize()
        assert torch.equal(out.cpu(), torch.cat([x[..., ::2, ::2], x[..., 1::2, ::2], x[..., ::2, 1::2], x[..., 1::2, 1::2]], 1))
        co.outside_untouched(f'space_to_depth ({fill})')
        cx.outside_untouched(f'space_to_depth input ({fill})')
        # 3x3 / 2 max pool, odd sizes
        for C, hw in ((88, (10, 10)), (24, (7, 9))):
            t = torch.randn(2, C, *hw, generator=g)
            Ho, Wo = (hw[0] - 1) // 2 + 1, (hw[1] - 1) // 2 + 1
            tv, ct = arena(2, C, *hw, C + 8, 4, dev, fill, data=t.to(dev))
            out, co = arena(2, C, Ho, Wo, C + 16, 12, dev, fill)
            _lib.check(L.mydet_maxpool3s2_f32(ops._ptr(tv), C + 8, ops._ptr(out), C + 16, 2, hw[0], hw[1], C, Ho, Wo, ops._stream()), 'maxpool3s2')
            torch.cuda.synchronize()
            assert torch.equal(out.cpu(), F.max_pool2d(t, 3, 2, 1))
            co.outside_untouched(f'maxpool3s2 ({fill})')
            ct.outside_untouched(f'maxpool3s2 input ({fill})')
        # channel sums: [B][S+1][C], slices 0..S-1 written
        t = torch.randn(2, 40, 9, 11, generator=g)
        S = ops.se_slices(9 * 11)
        tv, ct = arena(2, 40, 9, 11, 56, 12, dev, fill, data=t.to(dev))
        part, cp = arena(2, S * 40, 1, 1, (S + 1) * 40, 0, dev, fill)
        _lib.check(L.mydet_channel_sums_f32(ops._ptr(tv), 56, 2, 9, 11, 40, ops._ptr(part), S, ops._stream()), 'channel_sums')
        torch.cuda.synchronize()
        cp.view_defined('channel_sums')
        cp.outside_untouched(f'channel_sums ({fill})')
        ct.outside_untouched(f'channel_sums input ({fill})')
        torch.testing.assert_close(part.reshape(2, S, 40).sum(1).cpu().double(), t.double().sum(dim=(2, 3)), rtol=1e-5, atol=1e-4)


# ---------------------------------------------------------------------------------------------------- lr_tb box head
def test_footprint_lr_tb_levels(dev):
    """All five levels in one launch (ctypes: ops.lr_tb_levels allocates the outputs), each level's input a slice and its (l, t, r, b)
    output 4 channels of a wider arena; tolerance of tests/test_gpu_lr_tb.py (1e-5 of the reference's rms)."""
    from mydetection_amd import _lib, ops
    from _refs import lr_tb_layer_f64
    g = torch.Generator().manual_seed(37)
    B, C = 2, 88
    ws = [torch.randn(C, 1, 3, 3, generator=g), torch.randn(C, 1, 3, 3, generator=g), torch.randn(2, C, 1, 3, generator=g) * 0.3,
          torch.randn(2, generator=g), torch.randn(2, C, 3, 1, generator=g) * 0.3, torch.randn(2, generator=g)]
    lr0, tb0, lr1, blr, tb1, btb = ws
    wp = ops.pack_lr_tb(lr0, tb0, lr1, blr, tb1, btb).to(dev)
    xs = [torch.randn(B, C, h, wd, generator=g) for h, wd in ((40, 24), (20, 12), (10, 6), (5, 3), (3, 2))]

    def run(fill):
        arr = (_lib.LrTbLevel * len(xs))()
        keep = []
        for i, x in enumerate(xs):
            H, W = x.shape[2:]
            xv, cx = arena(B, C, H, W, C + 8, 4, dev, fill, data=x.to(dev))
            out, co = arena(B, 4, H, W, 12, 4, dev, fill)
            arr[i] = _lib.LrTbLevel(xv.data_ptr(), C + 8, wp.data_ptr(), out.data_ptr(), 12, H, W)
            keep.append((xv, cx, out, co))
        _lib.check(_lib.lib().mydet_lr_tb_levels_f32(len(xs), ctypes.cast(arr, ctypes.c_void_p), B, C, ops._stream()), 'mydet_lr_tb_levels_f32')
        torch.cuda.synchronize()
        for xv, cx, out, co in keep:
            co.view_defined('lr_tb output')
            co.outside_untouched(f'lr_tb output ({fill})')
            cx.outside_untouched(f'lr_tb input ({fill})')
        return [k[2].clone() for k in keep]

    ys = run('sentinel')
    for x, y in zip(xs, ys):
        ref = lr_tb_layer_f64(x, lr0, tb0, lr1, blr, tb1, btb).numpy()
        err = float(abs(y.cpu().numpy().astype('float64') - ref).max())
        rms = float((ref ** 2).mean() ** 0.5)
        assert err <= 1e-5 * rms, (tuple(x.shape), err, rms)
    for y, y0 in zip(ys, run('zero')):
        assert torch.equal(y, y0)


# ---------------------------------------------------------------------------------------------------- production compositions
def _randomise(mod, g):
    with torch.no_grad():
        for n, p_ in list(mod.named_parameters()) + list(mod.named_buffers()):
            if n.endswith('running_var'):
                p_.copy_(torch.rand(p_.shape, generator=g) + 0.5)
            elif n.endswith('num_batches_tracked'):
                continue
            elif p_.dim() == 4:
                p_.copy_(torch.randn(p_.shape, generator=g) / (p_.shape[1] * p_.shape[2] * p_.shape[3]) ** 0.5)
            else:
                p_.copy_(torch.randn(p_.shape, generator=g) * 0.3 + (1.0 if n.endswith('bn.weight') or n.endswith('.1.weight') else 0.0))
    return mod.eval()


@pytest.mark.parametrize('c,shortcut', [(192, True), (384, False)])
def test_footprint_bottleneck_csp_halves(dev, c, shortcut):
    """BottleneckCSP at YOLOv5-m's 40 x 40 shapes (hidden width 96 / 192, batch 8: past the smallest float32 tile): the block's output
    and EACH HALF of the concatenated buffer against its own float64 half (a half-write that clips the other half's first channels is
    averaged away by cv4 otherwise)."""
    from mydetection_amd.external.ultralytics.common import BottleneckCSP
    g = torch.Generator().manual_seed(41)
    csp = _randomise(BottleneckCSP(c, c, n=2, shortcut=shortcut), g)
    t = torch.randn(8, c, 40, 40, generator=g)

    def bn(z, m, sl=slice(None)):
        return F.batch_norm(z, m.running_mean.double()[sl], m.running_var.double()[sl], m.weight.double()[sl], m.bias.double()[sl], False, 0.0, m.eps)

    def conv_ref(z, m):
        return F.leaky_relu(bn(F.conv2d(z, m.conv.weight.double(), None, m.s, m.k // 2), m.bn), 0.1)

    td = t.double()
    h = conv_ref(td, csp.cv1)
    for b_ in csp.m:
        r = conv_ref(conv_ref(h, b_.cv1), b_.cv2)
        h = h + r if b_.add else r
    c_ = csp.c_
    half0 = F.leaky_relu(bn(F.conv2d(h, csp.cv3.weight.double()), csp.bn, slice(0, c_)), 0.1)
    half1 = F.leaky_relu(bn(F.conv2d(td, csp.cv2.weight.double()), csp.bn, slice(c_, 2 * c_)), 0.1)
    ref = conv_ref(torch.cat((half0, half1), 1), csp.cv4)
    csp = csp.to(dev)
    seen = []
    cv4_forward = csp.cv4.forward
    csp.cv4.forward = lambda z, *a, **kw: (seen.append(z), cv4_forward(z, *a, **kw))[1]
    y = csp(t.to(dev)).cpu().double()
    assert len(seen) == 1 and tuple(seen[0].shape) == (8, 2 * c_, 40, 40)
    cat = seen[0].cpu().double()
    for name, got, want in (('cv3 half', cat[:, :c_], half0), ('cv2 half', cat[:, c_:], half1)):
        err = (got - want).abs().max().item()
        assert err <= 3e-5 * want.abs().max().item(), (name, err)
    assert (y - ref).abs().max() <= 3e-5 * ref.abs().max()


@pytest.mark.parametrize('enable_conf', [False, True])
def test_footprint_head_with_center(dev, enable_conf):
    """EfDetHead_wCenter (registry 'effrpn_ct'), 80 classes, with and without the conf channel: raw['class'] / ['conf'] / ['center'] /
    ['bbox'] against the float64 composition of the head's own layers (oracle.efficientdet.head_with_center) at the head tolerance of
    the model tests (1e-4, 1e-4); the class and centerness convs write channel ranges of ONE pixel-major tensor and `packed` must name
    them.  With enable_conf the centerness range used to start at channel 81, 4 bytes past a 16-byte boundary."""
    from mydetection_amd import ops
    from mydetection_amd.models.rpns import EfDetHead_wCenter
    from oracle import efficientdet as oe
    n_cls, chs, sizes, B = 80, (88, 88, 88), ((12, 10), (6, 5), (3, 3)), 2
    cfg = {'general.num_class': n_cls, 'model.effrpn.num_anchor_per_level': 1, 'model.fpn.out_channels': chs, 'model.effrpn.repeat_num': 2,
           'model.effrpn.enable_centerscore': True, 'model.effrpn.enable_conf': enable_conf}
    g = torch.Generator().manual_seed(43)
    head = _randomise(EfDetHead_wCenter(cfg), g)
    with torch.no_grad():
        for n, p_ in head.named_parameters():
            if n.endswith('bias') and p_.dim() == 1 and ('class_nets' in n or 'center_nets' in n or 'bbox_lasts' in n):
                p_.copy_(torch.randn(p_.shape, generator=g))
    feats = [torch.randn(B, c, *hw, generator=g) for c, hw in zip(chs, sizes)]
    sd = {'rpn.' + k: v.double() for k, v in head.state_dict().items()}
    want = oe.head_with_center([f.double() for f in feats], sd, repeat=2)
    head = head.to(dev)
    with torch.no_grad():
        raws = head([f.to(dev).contiguous(memory_format=torch.channels_last) for f in feats])
    torch.cuda.synchronize()
    cls_ch = n_cls + 1 if enable_conf else n_cls
    for raw, (c_ref, b_ref, ct_ref) in zip(raws, want):
        c_ref, b_ref, ct_ref = (t.permute(0, 2, 3, 1) for t in (c_ref, b_ref, ct_ref))
        assert c_ref.shape[-1] == cls_ch
        pairs = [('bbox', b_ref), ('center', ct_ref), ('class', c_ref[..., 1:] if enable_conf else c_ref)]
        if enable_conf:
            pairs.append(('conf', c_ref[..., 0:1]))
        assert set(raw) == {k for k, _ in pairs}
        for key, ref in pairs:
            assert tuple(raw[key].shape) == tuple(ref.shape), key
            torch.testing.assert_close(raw[key].cpu().double(), ref, rtol=1e-4, atol=1e-4, msg=lambda m, key=key: f'{key}: {m}')
        both, ld, astride, cls_c0, conf_c0 = raw.packed['cls']                  # what the decode kernels read
        pix = both.permute(0, 2, 3, 1)
        assert ops.nhwc_ld(both) == ld and conf_c0 % 4 == 0 and cls_c0 == (1 if enable_conf else 0) and astride <= ld
        assert torch.equal(pix[..., conf_c0:conf_c0 + 1], raw['center']) and torch.equal(pix[..., cls_c0:cls_c0 + n_cls], raw['class'])
        if not enable_conf:                                                     # the shipped layout: unchanged
            assert (tuple(both.shape[1:2]), ld, astride, cls_c0, conf_c0) == ((81,), 84, 81, 0, 80)
    # the decode layer that reads `packed` in place ('FCOS': centerness from the head's own branch) == the same layer on plain copies of
    # the raw tensors (which it packs itself): the offsets `packed` names are the ones the kernel needs
    from mydetection_amd.models.detlayers.fcos import FCOSLayer
    lcfg = {'model.fcos.anchors': [0, 64, 128, 256], 'model.fpn.out_strides': (8, 16, 32), 'general.num_class': n_cls}
    for lvl, (raw, hw) in enumerate(zip(raws, sizes)):
        layer = FCOSLayer(lvl, lcfg)
        img = (hw[0] * layer.stride, hw[1] * layer.stride)
        got, _ = layer(raw, img)
        want_d, _ = layer({k: v.contiguous() for k, v in raw.items()}, img)
        for key in ('bbox', 'class_idx', 'score'):
            assert torch.equal(got[key], want_d[key]), (lvl, key)
        assert bool(torch.isfinite(got['score']).all()) and bool((got['score'] > 0).all())


# ---------------------------------------------------------------------------------------------------- depthwise / MBConv / stem + SE tail
def _dw_family_footprint(dev, kind, B, C, k, s, H, W, Cse, tail, unsupported=False):
    """One launch of mydet_dwconv_f32 ('dw'), mydet_mbconv_expand_dw_f32 ('mbconv', C = input channels, 6 C expanded) or
    mydet_stem_dw_f32 ('stem') through ctypes: input a slice (the stem's image: a channels-last slice read through element strides),
    y an arena; without the tail the squeeze partial sums [B,S+1,C] are an arena (slices 0..S-1 the launch's to define, slice S not
    its to touch), with it (`tail`: mydet_se_tail) the gate [B,C] is.  The share buffer `hpart` is the kernels' own protocol state
    (ops.se_shares: header + (value, epoch) pairs that only the launches may touch), so it is not poisoned; its launch counter must
    advance by one per launch, which also shows that the tail ran."""
    from mydetection_amd import _lib, ops
    from mydetection_amd.external.efficientnet.model import static_same_pad
    from _refs import act_f64, se_gate_f64
    L = _lib.lib()
    g = torch.Generator().manual_seed(1000 * C + 10 * H + k + s)
    if kind == 'dw':
        pad = static_same_pad(k, s, 240)
        Cg = C
        x = torch.randn(B, C, H, W, generator=g)
        wd = torch.randn(k, k, C, generator=g) / k
        sc, sh = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.3
        ref = F.conv2d(F.pad(x.double(), (pad[1], pad[3], pad[0], pad[2])), wd.double().permute(2, 0, 1).reshape(C, 1, k, k), None, s, 0, 1, C)
        ref = act_f64(ref * sc.double().view(1, -1, 1, 1) + sh.double().view(1, -1, 1, 1), 2)
        tol = 2e-5
        dv = [t.to(dev) for t in (wd, sc, sh)]
    elif kind == 'mbconv':
        pad = static_same_pad(k, s, 240)
        Cg = 6 * C
        x = torch.randn(B, C, H, W, generator=g)
        we = torch.randn(Cg, C, generator=g) / C ** 0.5
        wd = torch.randn(k, k, Cg, generator=g) / k
        sh0, sh1 = torch.randn(Cg, generator=g) * 0.3, torch.randn(Cg, generator=g) * 0.3
        e = act_f64(F.conv2d(x.double(), we.double().view(Cg, C, 1, 1)) + sh0.double().view(1, -1, 1, 1), 2)
        ref = F.conv2d(F.pad(e, (pad[1], pad[3], pad[0], pad[2])), wd.double().permute(2, 0, 1).reshape(Cg, 1, k, k), None, s, 0, 1, Cg)
        ref = act_f64(ref + sh1.double().view(1, -1, 1, 1), 2)
        tol = 2e-5 * max(1.0, ref.abs().max().item())
        dv = [t.to(dev) for t in (we.contiguous(), sh0, wd, sh1)]
    else:
        assert (C, k, s) == (32, 3, 1)
        pad = (1 if H % 2 else 0, 1 if W % 2 else 0, 1, 1)                          # TF "SAME" of the stride-2 stem conv
        Cg = 32
        x = torch.rand(B, 3, H, W, generator=g) * 2 - 1
        ws_ = torch.randn(32, 3, 3, 3, generator=g) * 0.3
        wd = torch.randn(3, 3, 32, generator=g) * 0.3
        sh0, sh1 = torch.randn(32, generator=g) * 0.2, torch.randn(32, generator=g) * 0.2
        t = act_f64(F.conv2d(F.pad(x.double(), (pad[1], pad[3], pad[0], pad[2])), ws_.double(), stride=2) + sh0.double().view(1, -1, 1, 1), 2)
        ref = act_f64(F.conv2d(t, wd.double().permute(2, 0, 1).reshape(32, 1, 3, 3), padding=1, groups=32) + sh1.double().view(1, -1, 1, 1), 2)
        tol = 3e-5 * max(1.0, ref.abs().max().item())
        dv = [t_.to(dev) for t_ in (ws_.permute(0, 2, 3, 1).contiguous(), sh0, wd, sh1)]
    Ho, Wo = ref.shape[2:]
    if kind == 'dw':
        S, groups = L.mydet_dwconv_slices(Ho, Wo, C, k, s), L.mydet_dwconv_se_groups(Ho, Wo, C, k, s)
    else:
        S = groups = L.mydet_mbconv_tiles(Ho, Wo, s if kind == 'mbconv' else 1)
    assert S >= 1 and groups >= 1
    se = None
    if tail:
        se = [t_.to(dev) for t_ in (torch.randn(Cse, Cg, generator=g) / Cg ** 0.5, torch.randn(Cse, generator=g) * 0.1,
                                    torch.randn(Cse, Cg, generator=g) * 0.3, torch.randn(Cg, generator=g) * 0.1)]
        hpart = ops.se_shares(dev, B * groups * Cse)
        hdr = hpart.view(torch.int32)[:_lib.SE_EPOCH_WORDS]

    def run(fill):
        cin = 3 if kind == 'stem' else C
        xin, cx = arena(B, cin, H, W, 8 if kind == 'stem' else cin + 16, 4, dev, fill, data=x.to(dev))
        out, co = arena(B, Cg, Ho, Wo, Cg + 24, 16, dev, fill)
        part = cp = gate = cg = st = None
        if tail:
            gate, cg = flat_arena(B * Cg, dev, fill)
            st = _lib.SeTail(se[0].data_ptr(), se[1].data_ptr(), se[2].data_ptr(), se[3].data_ptr(), gate.data_ptr(), hpart.data_ptr(), Cse,
                             hpart.numel() * 4)
            before = int(hdr[0])
        else:                   # [B][S+1][C] as a [B, S*C of (S+1)*C, 1, 1] map: the view is slices 0..S-1 of every image
            part, cp = arena(B, S * Cg, 1, 1, (S + 1) * Cg, 0, dev, fill)
        tail_arg = ctypes.byref(st) if st is not None else None
        if kind == 'dw':
            code = L.mydet_dwconv_f32(ops._ptr(xin), ops.nhwc_ld(xin), ops._ptr(dv[0]), ops._ptr(dv[1]), ops._ptr(dv[2]), ops._ptr(out),
                                      ops.nhwc_ld(out), B, H, W, C, k, s, pad[0], pad[1], Ho, Wo, ops.ACT_SWISH, ops._ptr(part), S, tail_arg,
                                      ops._stream())
        elif kind == 'mbconv':
            code = L.mydet_mbconv_expand_dw_f32(ops._ptr(xin), ops.nhwc_ld(xin), ops._ptr(dv[0]), ops._ptr(dv[1]), ops._ptr(dv[2]),
                                                ops._ptr(dv[3]), ops._ptr(out), ops.nhwc_ld(out), B, H, W, C, Cg, k, s, pad[0], pad[1], Ho, Wo,
                                                ops._ptr(part), S, tail_arg, ops._stream())
        else:
            sb, sc_, sh_, sw = xin.stride()
            code = L.mydet_stem_dw_f32(ops._ptr(xin), sb, sc_, sh_, sw, ops._ptr(dv[0]), ops._ptr(dv[1]), ops._ptr(dv[2]), ops._ptr(dv[3]),
                                       ops._ptr(out), ops.nhwc_ld(out), B, H, W, 32, pad[0], pad[1], Ho, Wo, ops._ptr(part), S, tail_arg,
                                       ops._stream())
        if unsupported:         # MYDET_E_UNSUPP is decided on the host before any launch: nothing at all may have been written
            torch.cuda.synchronize()
            assert code == -2, code
            assert co.undefined_in_view()[0] == out.numel() and cg.undefined_in_view()[0] == gate.numel() and int(hdr[0]) == before
            for c in (co, cx, cg):
                c.outside_untouched(f'{kind} declined launch ({fill})')
            return None, None
        _lib.check(code, f'{kind} launch')
        torch.cuda.synchronize()
        co.view_defined(f'{kind} output ({fill})')
        co.outside_untouched(f'{kind} output ({fill})')
        cx.outside_untouched(f'{kind} input ({fill})')
        if tail:
            cg.view_defined(f'{kind} gate ({fill})')
            cg.outside_untouched(f'{kind} gate ({fill})')
            assert int(hdr[0]) == before + 1 and int(hdr[1]) == 0 and int(hdr[2]) == 0, hdr[:3].tolist()
            return out.clone(), gate.view(B, Cg).clone()
        cp.view_defined(f'{kind} squeeze sums ({fill})')
        cp.outside_untouched(f'{kind} squeeze sums ({fill})')
        return out.clone(), part.reshape(B, S, Cg).sum(1)

    y, extra = run('sentinel')
    if unsupported:
        return
    err = (y.cpu().double() - ref).abs().max().item()
    print(f'{kind} C={C} k={k} s={s} {H}x{W} tail={tail}: err {err:.3e} tol {tol:.3e}')
    assert err <= tol
    if tail:
        gerr = (extra.cpu().double() - se_gate_f64(y.cpu(), *[t_.cpu() for t_ in se])).abs().max().item()
        assert gerr < 3e-6, gerr
    else:
        torch.testing.assert_close(extra.cpu().double(), y.cpu().double().sum(dim=(2, 3)), rtol=1e-5, atol=1e-3)
    y0, extra0 = run('zero')
    assert torch.equal(y, y0) and torch.equal(extra, extra0)


@pytest.mark.parametrize('C,Cse,k,s,H,W', [(1152, 48, 5, 1, 20, 20),     # LDS-tiled kernel, 36 channel chunks
                                           (144, 6, 3, 1, 37, 41),       # ragged tiles, a last chunk of 16 channels
                                           (16, 4, 3, 1, 64, 96),        # the narrow tile
                                           (672, 28, 5, 2, 40, 40),      # stride 2: the slice kernel, asymmetric SAME pad
                                           (240, 10, 3, 2, 31, 33)])     # stride 2, odd sizes
def test_footprint_dwconv_se_tail(dev, C, Cse, k, s, H, W):
    _dw_family_footprint(dev, 'dw', 2, C, k, s, H, W, Cse, tail=True)


@pytest.mark.parametrize('tail', [False, True])
@pytest.mark.parametrize('k,s,cin,hw', [(3, 2, 16, (40, 48)), (3, 1, 24, (24, 32)), (5, 2, 24, (22, 26)), (5, 1, 40, (17, 23)),
                                        (3, 2, 40, (16, 16))])
def test_footprint_mbconv_expand_dw(dev, k, s, cin, hw, tail):
    """The five instantiated (K, stride, Cin) forms, static-SAME pads (asymmetric at stride 2), with the squeeze sums and with the tail.
    (5, 1, 40) with the tail needs more than the 80 KiB of LDS the launcher allows and is declined with MYDET_E_UNSUPP (the blocks use
    the fused launch for (3,2,16), (3,1,24), (5,2,24) only: ops.MBCONV_FUSED_SHAPES): a declined launch must write nothing."""
    _dw_family_footprint(dev, 'mbconv', 2, cin, k, s, hw[0], hw[1], max(4, cin // 4), tail=tail,
                         unsupported=tail and (k, s, cin) == (5, 1, 40))


@pytest.mark.parametrize('tail', [False, True])
@pytest.mark.parametrize('H,W', [(64, 64), (61, 95)])
def test_footprint_stem_dw(dev, H, W, tail):
    _dw_family_footprint(dev, 'stem', 2, 32, 3, 1, H, W, 8, tail=tail)


def test_footprint_conv_stem(dev):
    """mydet_conv2d_stem_f32 (ctypes: ops.conv2d_stem allocates y): the image a channels-last slice read through element strides."""
    from mydetection_amd import _lib, ops
    g = torch.Generator().manual_seed(47)
    for s, pad, (H, W) in ((1, (1, 1, 1, 1), (34, 38)), (2, (0, 0, 1, 1), (34, 38)), (2, (1, 1, 1, 1), (33, 37))):
        x = torch.rand(2, 3, H, W, generator=g)
        w = torch.randn(32, 3, 3, 3, generator=g) * 0.2
        scale, shift = torch.rand(32, generator=g) + 0.5, torch.randn(32, generator=g) * 0.1
        ref = F.conv2d(F.pad(x, (pad[1], pad[3], pad[0], pad[2])).double(), w.double(), None, s)
        ref = F.leaky_relu(ref * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1), 0.1)
        Ho, Wo = ref.shape[2:]
        wd, scd, shd = w.permute(0, 2, 3, 1).contiguous().to(dev), scale.to(dev), shift.to(dev)

        def run(fill):
            xin, cx = arena(2, 3, H, W, 8, 4, dev, fill, data=x.to(dev))
            out, co = arena(2, 32, Ho, Wo, 56, 12, dev, fill)
            sb, sc_, sh_, sw = xin.stride()
            _lib.check(_lib.lib().mydet_conv2d_stem_f32(ops._ptr(xin), sb, sc_, sh_, sw, ops._ptr(wd), ops._ptr(scd), ops._ptr(shd), ops._ptr(out), 56,
                                                        2, H, W, 32, s, pad[0], pad[1], Ho, Wo, ops.ACT_LEAKY, ops._stream()), 'mydet_conv2d_stem_f32')
            torch.cuda.synchronize()
            co.view_defined('conv_stem output')
            co.outside_untouched(f'conv_stem output ({fill})')
            cx.outside_untouched(f'conv_stem input ({fill})')
            return out.clone()
        y = run('sentinel')
        assert (y.cpu().double() - ref).abs().max() < 1e-5
        assert torch.equal(run('zero'), y)
