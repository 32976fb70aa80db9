"""mydet_conv_stem_p3_f32 (csrc/conv_stem_p3.hip): Darknet-53's stem and its first stride-2 conv as one launch.

Shapes: the smallest at which each mechanism can go wrong -- whole tiles (64 x 64), ragged 8 x 16 tiles in both directions (40 x 72:
the stride-2 output is 20 x 36), odd sizes whose last patch row and column lie outside the image (37 x 51), one tile per image with
image borders on all four sides (16 x 32), two channel tiles (Cout 128); the image as a contiguous NCHW tensor and as a channels-last
view, the output dense and inside a wider buffer (ldy = Cout + 8).
Bars: 2e-5 * max|y| against the float64 chain (the split-bf16 family's bar, tests/test_gpu_kernels.py), and the family's pair bar
against the two-launch path (4 x its float64 error + 1e-6).  The two-launch path itself is held to the first bar on the same inputs
(the negative control: the bar tests the fused kernel, not the inputs).
The stem shift is positive for every channel, so act(shift) != 0: a kernel that fills the second conv's padding ring with act(shift)
instead of 0 is off by O(shift * |w|) ~ 0.1 at every border pixel, four orders above the bar (checked by hand: replacing the ring's 0
with act(shift) in the kernel fails test_border_pixels_see_zero_padding and test_vs_float64 on every shape).
"""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from _arena import arena

pytestmark = pytest.mark.gpu

# (B, H, W, Cout, channels-last image, ldy - Cout)
CASES = [(2, 64, 64, 64, False, 0), (2, 40, 72, 64, True, 8), (1, 37, 51, 64, False, 8), (3, 16, 32, 64, True, 0),
         (2, 40, 72, 128, False, 8)]
IDS = [f'B{c[0]}_{c[1]}x{c[2]}_c{c[3]}{"_cl" if c[4] else ""}{"_wide" if c[5] else ""}' for c in CASES]


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    from mydetection_amd import _lib
    _lib.lib()                                   # fail loudly if the HIP library is missing
    return torch.device('cuda:0')


_MADE = {}


def _case(dev, case):
    """Inputs, device operands and the float64 reference of one case: computed once, shared, never modified."""
    if case in _MADE:
        return _MADE[case]
    from mydetection_amd import ops
    B, H, W, Cout, _, _ = case
    g = torch.Generator().manual_seed(1000 * H + W + Cout)
    x = torch.rand(B, 3, H, W, generator=g)
    w0 = torch.randn(32, 3, 3, 3, generator=g) / 27 ** 0.5
    sc0, sh0 = torch.rand(32, generator=g) + 0.5, torch.rand(32, generator=g) * 0.4 + 0.1      # shift > 0: act(shift) != 0
    w1 = torch.randn(Cout, 32, 3, 3, generator=g) / 288 ** 0.5
    sc1, sh1 = torch.rand(Cout, generator=g) + 0.5, torch.randn(Cout, generator=g) * 0.1
    mid = F.conv2d(F.pad(x.double(), (1, 1, 1, 1)), w0.double())
    mid = F.leaky_relu(mid * sc0.double().view(1, -1, 1, 1) + sh0.double().view(1, -1, 1, 1), 0.1)
    ref = F.conv2d(F.pad(mid, (1, 1, 1, 1)), w1.double(), None, 2)
    ref = F.leaky_relu(ref * sc1.double().view(1, -1, 1, 1) + sh1.double().view(1, -1, 1, 1), 0.1)
    w0d = w0.permute(0, 2, 3, 1).contiguous().to(dev)
    w1d = w1.permute(0, 2, 3, 1).contiguous().to(dev)
    d = dict(x=x, ref=ref, w0d=w0d, w1d=w1d, w0p=ops.stem_p3_weights(w0d), w1p=ops.split_bf16(w1d), sc0=sc0.to(dev), sh0=sh0.to(dev),
             sc1=sc1.to(dev), sh1=sh1.to(dev))
    _MADE[case] = d
    return d


def _image(dev, d, channels_last):
    x = d['x'].to(dev)
    if channels_last:
        x = x.contiguous(memory_format=torch.channels_last)
        assert x.stride(1) == 1
    return x


def _fused(dev, d, case, x=None, out=None):
    from mydetection_amd import ops
    _, _, _, Cout, cl, extra = case
    x = _image(dev, d, cl) if x is None else x
    y = ops.conv_stem_p3(x, d['w0p'], d['sc0'], d['sh0'], (1, 1, 1, 1), d['w1p'], d['sc1'], d['sh1'], out=out,
                         out_ld=Cout + extra if out is None else None)
    assert y is not None
    return y


def _two_launches(dev, d, case):
    from mydetection_amd import ops
    mid = ops.conv2d_stem(_image(dev, d, case[4]), d['w0d'], d['sc0'], d['sh0'], 1, (1, 1, 1, 1), ops.ACT_LEAKY)
    y = ops.conv3x3_p3(mid, d['w1p'], d['sc1'], d['sh1'], 2, ops.ACT_LEAKY)
    assert y is not None
    return y


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_vs_float64_and_two_launches(dev, case):
    from mydetection_amd import ops
    d = _case(dev, case)
    ref = d['ref']
    ops.TIMER = ops.KernelTimer()
    try:
        y = _fused(dev, d, case)
    finally:
        timer, ops.TIMER = ops.TIMER, None
    assert set(timer.spans) == {'conv_stem_p3'} and len(timer.spans['conv_stem_p3']) == 1
    assert tuple(y.shape) == tuple(ref.shape) and ops.nhwc_ld(y) == case[3] + case[5]
    y2 = _two_launches(dev, d, case)
    tol = 2e-5 * ref.abs().max().item()
    e1, e2 = (y.cpu().double() - ref).abs().max().item(), (y2.cpu().double() - ref).abs().max().item()
    print(f'{case}: fused {e1:.3e}  two launches {e2:.3e}  bar {tol:.3e}')
    assert e2 <= tol, ('the two-launch path misses the bar on these inputs', e2, tol)
    assert e1 <= tol, (e1, e2, tol)
    assert (y - y2).abs().max().item() <= 4.0 * e2 + 1e-6, ((y - y2).abs().max().item(), e2)


@pytest.mark.parametrize('case', CASES[1:4], ids=IDS[1:4])
def test_border_pixels_see_zero_padding(dev, case):
    """The stem pixels around the stem map are the second conv's padding: 0, not act(shift)."""
    d = _case(dev, case)
    y, ref = _fused(dev, d, case).cpu().double(), d['ref']
    assert F.leaky_relu(d['sh0'], 0.1).abs().min().item() > 0.05
    border = torch.zeros(ref.shape[2:], dtype=torch.bool)
    border[0], border[-1], border[:, 0], border[:, -1] = True, True, True, True
    err = (y - ref).abs()[:, :, border].max().item()
    assert err <= 2e-5 * ref.abs().max().item(), err


@pytest.mark.parametrize('case', [CASES[1], CASES[2]], ids=[IDS[1], IDS[2]])
def test_repeatable_and_graph_replay(dev, case):
    d = _case(dev, case)
    x = _image(dev, d, case[4])
    a = _fused(dev, d, case, x=x).clone()
    assert torch.equal(_fused(dev, d, case, x=x), a)
    from mydetection_amd import ops
    out, _ = ops.empty_nhwc(*a.shape, dev, ld=case[3] + case[5])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _fused(dev, d, case, x=x, out=out)       # function attributes are set outside the capture
    torch.cuda.current_stream().wait_stream(side)
    out.zero_()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _fused(dev, d, case, x=x, out=out)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, a)


@pytest.mark.parametrize('case', [CASES[2], CASES[4]], ids=[IDS[2], IDS[4]])
def test_footprint(dev, case):
    """Image and output inside poisoned arenas: nothing outside the output view changes, and NaN surroundings give the bits that zero
    surroundings give."""
    B, H, W, Cout, _, _ = case
    d = _case(dev, case)
    Ho, Wo = d['ref'].shape[2:]

    def run(fill):
        xin, cx = arena(B, 3, H, W, 8, 4, dev, fill, data=d['x'].to(dev))
        out, co = arena(B, Cout, Ho, Wo, Cout + 28, 12, dev, fill)
        _fused(dev, d, case, x=xin, out=out)
        torch.cuda.synchronize()
        co.view_defined('conv_stem_p3 output')
        co.outside_untouched(f'conv_stem_p3 output ({fill})')
        cx.outside_untouched(f'conv_stem_p3 input ({fill})')
        return out.clone()
    y = run('sentinel')
    assert (y.cpu().double() - d['ref']).abs().max().item() <= 2e-5 * d['ref'].abs().max().item()
    assert torch.equal(run('zero'), y)


def test_unsupported_arguments_launch_nothing(dev):
    from mydetection_amd import _lib, ops
    case = CASES[3]
    d = _case(dev, case)
    B, H, W, Cout, _, _ = case
    x = _image(dev, d, False)
    Ho, Wo = d['ref'].shape[2:]
    out, co = arena(B, Cout, Ho, Wo, Cout + 8, 0, dev)
    sb, sc, sh, sw = x.stride()
    null = ctypes.c_void_p(0)

    def call(**kw):
        a = dict(x=ops._ptr(x), w0=ops._ptr(d['w0p']), w1=ops._ptr(d['w1p']), y=ops._ptr(out), ldy=Cout + 8, C0=32, Cout=Cout, s0=1, s1=2,
                 act0=1, act1=1, B=B)
        a.update(kw)
        return _lib.lib().mydet_conv_stem_p3_f32(a['x'], sb, sc, sh, sw, a['w0'], ops._ptr(d['sc0']), ops._ptr(d['sh0']), a['act0'], a['w1'],
                                                 ops._ptr(d['sc1']), ops._ptr(d['sh1']), a['act1'], a['y'], a['ldy'], a['B'], H, W, a['C0'],
                                                 a['Cout'], a['s0'], 1, 1, H, W, a['s1'], ops._stream())
    assert call(x=null) == -1 and call(w0=null) == -1 and call(w1=null) == -1 and call(y=null) == -1 and call(B=0) == -1
    assert call(C0=16) == -2 and call(Cout=48) == -2 and call(s0=2) == -2 and call(s1=1) == -2
    assert call(act0=ops.ACT_SWISH) == -2 and call(act1=ops.ACT_SWISH) == -2
    assert call(ldy=Cout - 4) == -1 and call(ldy=Cout + 2) == -1
    assert call(y=ctypes.c_void_p(out.data_ptr() + 4)) == -1
    assert call(w1=ctypes.c_void_p(d['w1p'].data_ptr() + 8)) == -1
    torch.cuda.synchronize()
    assert co.undefined_in_view()[0] == B * Cout * Ho * Wo          # nothing was launched: the view is still poison
    co.outside_untouched('refused calls')
    assert call() == 0
    torch.cuda.synchronize()
    co.view_defined('accepted call')
