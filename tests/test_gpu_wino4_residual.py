"""GPU: the residual path of the Winograd F(4x4,3x3) GEMM kernel (csrc/conv_wino4.hip, conv_wino4_kernel<ACT, true>).

The residual is fetched in two halves -- output rows 0-1 under the peeled last K stage, rows 2-3 after the column pass of the
output transform -- and added with one float32 add of its own after the activation.  So a launch with `residual=` must equal the
same launch without it plus the residual, bit for bit (torch.equal, no tolerance): any residual quad that is consumed before it has
landed, lands in the wrong register or belongs to the wrong pixel shows as a difference.

  Cin   4, 8, 12, 16, 64: nk = 1, 2, 3, 4, 16 K stages -- the peeled last stage alone, behind one looped stage, and deep loops
  Cout  4, 32, 36, 96: a partial channel block, a whole one, two waves' halves with the second partial, three blocks
  maps  6 x 10 at B = 3 (ragged tile rows AND columns: 18 tiles) and 4 x 4 at B = 40 (a 32-tile block spans 32 images, the
        second block has 8 tiles)
  views the residual is a channel slice of a wider tensor (ldr != ldy) and y a channel slice of a wider one (ldy > Cout); the
        channels around the output slice hold a sentinel and must come back untouched
Against float64: the bound of tests/test_gpu_kernels.py (_conv_case with wino4=True: 6e-5 * max(1, max|ref|)), on two of the shapes.
The K-cut tail (pieces + wino4_fixup_kernel add the residual for the tail items) gets the same identity on a shape the launcher's
own plan cuts on the running chip; the same launch eight times is bit-equal."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

SENTINEL = -12345.75
CINS, COUTS = (4, 8, 12, 16, 64), (4, 32, 36, 96)
MAPS = {'6x10_ragged': (3, 6, 10), '4x4_b40': (40, 4, 4)}
W4_TOL = 6e-5                       # tests/test_gpu_kernels.py::_conv_case, wino4=True: tol = 6e-5 * max(1, max|ref|)


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    from mydetection_amd import _lib
    _lib.lib()                                   # fail loudly if the HIP library is missing
    return torch.device('cuda:0')


def _slice_view(B, C, H, W, ld, c0, dev, data=None):
    """Logical [B, C, H, W] view = channels c0 .. c0 + C of a [B, H, W, ld] buffer filled with the sentinel."""
    buf = torch.full((B, H, W, ld), SENTINEL, dtype=torch.float32, device=dev)
    view = buf.permute(0, 3, 1, 2)[:, c0:c0 + C]
    if data is not None:
        view.copy_(data)
    return buf, view


def _inputs(B, Cin, Cout, H, W, dev, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / (Cin * 9) ** 0.5
    scale = torch.rand(Cout, generator=g) + 0.5
    shift = torch.randn(Cout, generator=g) * 0.1
    res = torch.randn(B, Cout, H, W, generator=g)
    return x, w, scale, shift, res


def _pair(dev, B, Cin, Cout, H, W, act, seed, views=True):
    """(y without residual, y with residual, residual on the device, host inputs) of one F(4x4) layer."""
    from mydetection_amd import ops
    x, w, scale, shift, res = _inputs(B, Cin, Cout, H, W, dev, seed)
    xd = x.to(dev).contiguous(memory_format=torch.channels_last)
    wd = w.permute(0, 2, 3, 1).contiguous().to(dev)
    u4 = ops.wino4_weights(wd)
    assert u4 is not None and ops.WINOGRAD and ops.WINOGRAD4
    sc, sh = scale.to(dev), shift.to(dev)
    if views:
        ldy, c0y = Cout + 24, 8
        _, rview = _slice_view(B, Cout, H, W, Cout + 12, 4, dev, data=res.to(dev))
        assert ops.nhwc_ld(rview) == Cout + 12
    else:
        rview = res.to(dev).contiguous(memory_format=torch.channels_last)
    outs = []
    for r in (None, rview):
        if views:
            buf, out = _slice_view(B, Cout, H, W, ldy, c0y, dev)
            assert ops.nhwc_ld(out) == ldy
            y = ops.conv2d(xd, wd, sc, sh, 3, 1, (1, 1, 1, 1), act, residual=r, out=out, wino4=u4)
            torch.cuda.synchronize()
            assert y.data_ptr() == out.data_ptr()
            assert bool((buf[..., :c0y] == SENTINEL).all()) and bool((buf[..., c0y + Cout:] == SENTINEL).all()), \
                f'{Cin}->{Cout}: channels outside the output slice were written'
            assert not bool((out == SENTINEL).any()), f'{Cin}->{Cout}: part of the output slice was not written'
        else:
            y = ops.conv2d(xd, wd, sc, sh, 3, 1, (1, 1, 1, 1), act, residual=r, wino4=u4)
        outs.append(y.contiguous(memory_format=torch.channels_last).clone())
    return outs[0], outs[1], rview, (x, w, scale, shift, res)


def _fp64(x, w, scale, shift, res, act):
    ref = F.conv2d(x.double(), w.double(), None, 1, 1) * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1)
    if act == 1:
        ref = F.leaky_relu(ref, 0.1)
    elif act == 2:
        ref = ref * torch.sigmoid(ref)
    return ref + res.double()


@pytest.mark.parametrize('act', [0, 1, 2], ids=['none', 'leaky', 'swish'])
@pytest.mark.parametrize('shape', list(MAPS))
def test_wino4_residual_is_one_add_after_the_activation(dev, shape, act):
    B, H, W = MAPS[shape]
    for Cin in CINS:
        for Cout in COUTS:
            plain, withres, r, _ = _pair(dev, B, Cin, Cout, H, W, act, seed=100 * Cin + Cout + act)
            want = plain + r
            assert torch.equal(withres, want), (
                f'{shape} {Cin}->{Cout} act {act}: {int((withres != want).sum())} of {want.numel()} outputs differ from (launch without '
                f'residual) + residual, max |diff| {(withres - want).abs().max().item():.3e}')


@pytest.mark.parametrize('case', [dict(shape='6x10_ragged', Cin=12, Cout=36, act=2), dict(shape='4x4_b40', Cin=64, Cout=96, act=1)],
                         ids=['6x10_12to36_swish', '4x4_b40_64to96_leaky'])
def test_wino4_residual_vs_fp64(dev, case):
    B, H, W = MAPS[case['shape']]
    _, withres, _, host = _pair(dev, B, case['Cin'], case['Cout'], H, W, case['act'], seed=17)
    ref = _fp64(*host, case['act'])
    tol = W4_TOL * max(1.0, ref.abs().max().item())
    err = (withres.cpu().double() - ref).abs().max().item()
    print(f'wino4 residual {case}: err {err:.3e} = {err / tol:.3f} of the bound {tol:.3e}')
    assert err <= tol, f'{case}: {err} > {tol}'


def _tail_shape(dev):
    """The first batch size at which the launcher's own plan cuts 64 -> 512 at 32 x 32 along K on this chip (B = 17 on 256 CUs)."""
    from mydetection_amd import _lib
    slots = 2 * torch.cuda.get_device_properties(dev).multi_processor_count
    out = (ctypes.c_int32 * 17)()
    for B in range(1, 129):
        if _lib.lib().mydet_wino4_tail_plan(B, 32, 32, 64, 512, slots, ctypes.cast(out, ctypes.c_void_p)) >= 1:
            return B, list(out)
    raise AssertionError(f'no batch size up to 128 gives 64 -> 512 at 32 x 32 a K-cut tail on {slots} workgroup slots')


def test_wino4_residual_kcut_tail_is_one_add(dev, monkeypatch):
    from mydetection_amd import _lib
    B, plan = _tail_shape(dev)
    assert plan[1] >= 1 and plan[5] >= 2, plan
    plain, withres, r, _ = _pair(dev, B, 64, 512, 32, 32, 1, seed=23, views=False)
    want = plain + r
    assert torch.equal(withres, want), f'B = {B}, plan {plan[:7]}: {int((withres != want).sum())} outputs differ from (launch without residual) + residual'
    monkeypatch.setenv('MYDET_W4_TAIL', '0')              # the tail did run: the uncut launch sums in another association
    _lib.lib().mydet_wino4_reload_tuning()
    try:
        uncut = _pair(dev, B, 64, 512, 32, 32, 1, seed=23, views=False)[1]
    finally:
        monkeypatch.delenv('MYDET_W4_TAIL')
        _lib.lib().mydet_wino4_reload_tuning()
    assert not torch.equal(withres, uncut), 'the tail rule did not trigger on a shape chosen to trigger it'


def test_wino4_residual_repeatable(dev):
    """128 -> 256 at 20 x 20, B = 8: 200 tiles x 8 channel blocks, 32 K stages; eight launches, bit-equal."""
    from mydetection_amd import ops
    B, Cin, Cout, H, W = 8, 128, 256, 20, 20
    x, w, scale, shift, res = _inputs(B, Cin, Cout, H, W, dev, seed=31)
    xd = x.to(dev).contiguous(memory_format=torch.channels_last)
    wd = w.permute(0, 2, 3, 1).contiguous().to(dev)
    rd = res.to(dev).contiguous(memory_format=torch.channels_last)
    sc, sh = scale.to(dev), shift.to(dev)
    u4 = ops.wino4_weights(wd)
    outs = [ops.conv2d(xd, wd, sc, sh, 3, 1, (1, 1, 1, 1), 1, residual=rd, wino4=u4).clone() for _ in range(8)]
    for i, o in enumerate(outs[1:], 1):
        assert torch.equal(o, outs[0]), f'launch {i} differs from launch 0 in {int((o != outs[0]).sum())} values'
