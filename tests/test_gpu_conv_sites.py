"""Every call site of ops.conv2d in the model code hands it the weight forms it always did, and gets the same bits.

Each module class runs on a 2 x 32 x 16 x 24 map (4 x 4 and 8 x 16 tiles ragged in one direction) with synthetic weights, once with the
launch thresholds down -- so that this small layer reaches the site's first-choice launchers -- and once with the shipped ones.  For every
ops.conv2d call the module makes: the forms it holds are the ones stated here (what the site passed before conv_forms / conv_route
existed), the KernelTimer family is the one ops.conv_route names, and the output is bit-equal to a direct ops.conv2d call on the same
prepared weight with those forms derived afresh."""
import pytest
import torch

pytestmark = pytest.mark.gpu

B, H, W, CIN, COUT = 2, 16, 24, 32, 64
LOW = dict(P3_MIN_WGS=1, P3_MIN_FILL=0.0, WINO4_MIN_ITEMS=1, B3_MIN_ROWS=1, B3_MIN_FLOP=0.0, B3_EXPAND_MIN_ROWS=1, B3_GATED_MIN_ROWS=1)


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda', 0)


def _module(m, dev):
    from mydetection_amd import synth
    m.load_state_dict(synth.make_state_dict(m.state_dict()), strict=True)
    return m.eval().to(dev)


def _input(dev, c=CIN, seed=0):
    from mydetection_amd import ops
    g = torch.Generator().manual_seed(seed)
    return ops.to_nhwc(torch.randn(B, c, H, W, generator=g).to(dev))[0]           # channels-last, as every feature map of the models


def _run(monkeypatch, thresholds, run, expected, view_of_last=False):
    """run() under a spy on ops.conv2d; expected: per conv call (forms held, b3_min_rows, family at the low thresholds, at the shipped).
    Returns run()'s tensor: the last conv call's output (view_of_last: its leading channels)."""
    from mydetection_amd import ops
    for name, value in (LOW.items() if thresholds == 'low' else ()):
        monkeypatch.setattr(ops, name, value)
    real, calls = ops.conv2d, []

    def spy(*args, **kw):
        ops.TIMER = ops.KernelTimer()
        try:
            y = real(*args, **kw)
        finally:
            timer, ops.TIMER = ops.TIMER, None
        calls.append((args, kw, y, list(timer.spans)))
        return y
    monkeypatch.setattr(ops, 'conv2d', spy)
    with torch.no_grad():
        out = run()
    monkeypatch.setattr(ops, 'conv2d', real)
    assert len(calls) == len(expected)
    for (args, kw, y, families), (forms, min_rows, low, shipped) in zip(calls, expected):
        x, w, scale, shift, k, stride, pad, act = args
        assert {f for f in ops.CONV_FORMS if kw.get(f) is not None} == set(forms), (forms, sorted(kw))
        assert kw.get('b3_min_rows') == min_rows
        ldr = ops.nhwc_ld(kw['residual']) if kw.get('residual') is not None else 0
        route = ops.conv_route(*x.shape[0:1], *x.shape[2:4], x.shape[1], w.shape[0], k, stride, pad, act, gated=kw.get('gate') is not None,
                               ldy=ops.nhwc_ld(y), ldr=ldr, forms=set(forms), b3_min_rows=min_rows)
        assert families == [route[0]] == [low if thresholds == 'low' else shipped], (families, route)
        fresh = {f: ops.CONV_FORM_WEIGHTS[f](w) for f in forms}
        direct = real(x, w, scale, shift, k, stride, pad, act, residual=kw.get('residual'), gate=kw.get('gate'), b3_min_rows=min_rows, **fresh)
        torch.cuda.synchronize()
        assert torch.equal(y, direct), route
    last = calls[-1][2]
    assert out.data_ptr() == last.data_ptr() and torch.equal(out, last[:, :out.shape[1]] if view_of_last else last)
    return out


@pytest.mark.parametrize('thresholds', ['low', 'shipped'])
@pytest.mark.parametrize('k,s,cin,cout,residual,forms,low,shipped', [
    (1, 1, CIN, COUT, False, ('b3',), 'conv_igemm', 'conv_igemm'),                    # 1x1 below 128 output channels
    (1, 1, CIN, 128, False, ('b3',), 'conv_igemm_b3', 'conv_igemm'),
    (3, 1, CIN, COUT, True, ('wino', 'b3'), 'conv_p3', 'conv_wino'),                  # below F(4x4)'s input channels
    (3, 1, 64, COUT, True, ('wino', 'wino4'), 'conv_wino4', 'conv_wino'),
    (3, 1, 40, COUT, False, ('wino',), 'conv_wino', 'conv_wino'),                     # Cin % 16: no planes
    (3, 2, CIN, COUT, False, ('b3',), 'conv_p3', 'conv_igemm'),
    (3, 2, 36, COUT, False, (), 'conv_igemm', 'conv_igemm'),
])
def test_conv_bn_leaky(dev, monkeypatch, thresholds, k, s, cin, cout, residual, forms, low, shipped):
    from mydetection_amd.models.modules import ConvBnLeaky
    m = _module(ConvBnLeaky(cin, cout, k, s), dev)
    x = _input(dev, cin)
    res = _input(dev, cout, seed=1) if residual else None
    _run(monkeypatch, thresholds, lambda: m(x, residual=res), [(forms, None, low, shipped)])


def test_conv_bn_leaky_without_p3(dev, monkeypatch):
    """The stride-2 layer with conv_p3 off, then with the split-bf16 kernels off: the next launcher of the ladder each time."""
    from mydetection_amd import ops
    from mydetection_amd.models.modules import ConvBnLeaky
    m = _module(ConvBnLeaky(CIN, COUT, 3, 2), dev)
    x = _input(dev)
    monkeypatch.setattr(ops, 'CONV_P3', False)
    _run(monkeypatch, 'low', lambda: m(x), [(('b3',), None, 'conv_igemm_b3', None)])
    monkeypatch.setattr(ops, 'SPLIT_BF16', False)
    _run(monkeypatch, 'low', lambda: m(x), [((), None, 'conv_igemm', None)])


@pytest.mark.parametrize('thresholds', ['low', 'shipped'])
@pytest.mark.parametrize('k,p,cin,forms,low,shipped', [(3, 1, CIN, ('wino',), 'conv_wino', 'conv_wino'),
                                                      (3, 1, 88, ('wino', 'wino4'), 'conv_wino4', 'conv_wino'),
                                                      (1, 0, CIN, (), 'conv_igemm', 'conv_igemm')])
def test_conv_bn(dev, monkeypatch, thresholds, k, p, cin, forms, low, shipped):
    from mydetection_amd.models.modules import ConvBn
    m = _module(ConvBn(cin, COUT, k, p), dev)
    x = _input(dev, cin)
    _run(monkeypatch, thresholds, lambda: m(x), [(forms, None, low, shipped)])


@pytest.mark.parametrize('thresholds', ['low', 'shipped'])
@pytest.mark.parametrize('k,s,cin,forms,low,shipped', [(3, 1, CIN, ('wino',), 'conv_wino', 'conv_wino'),
                                                      (3, 1, 64, ('wino', 'wino4'), 'conv_wino4', 'conv_wino'),
                                                      (3, 2, CIN, (), 'conv_igemm', 'conv_igemm'),
                                                      (1, 1, CIN, (), 'conv_igemm', 'conv_igemm')])
def test_ultralytics_conv(dev, monkeypatch, thresholds, k, s, cin, forms, low, shipped):
    from mydetection_amd.external.ultralytics.common import Conv
    m = _module(Conv(cin, COUT, k, s), dev)
    x = _input(dev, cin)
    res = _input(dev, COUT, seed=1) if s == 1 else None
    _run(monkeypatch, thresholds, lambda: m(x, residual=res), [(forms, None, low, shipped)])


@pytest.mark.parametrize('thresholds', ['low', 'shipped'])
def test_mbconv_block(dev, monkeypatch, thresholds):
    """Expand conv (32 -> 192, swish) and gated project conv (192 -> 64): split-bf16 planes with the block's own row thresholds."""
    from mydetection_amd import ops
    from mydetection_amd.external.efficientnet.model import BlockArgs, GlobalParams, MBConvBlock
    m = _module(MBConvBlock(BlockArgs(3, 1, CIN, COUT, 6, True, 1, 0.25), GlobalParams(0.99, 1e-3, 0.2, 1.0, 1.0, 8, 240)), dev)
    x = _input(dev)
    expand_rows, gated_rows = (1, 1) if thresholds == 'low' else (ops.B3_EXPAND_MIN_ROWS, ops.B3_GATED_MIN_ROWS)
    _run(monkeypatch, thresholds, lambda: m(x), [(('b3',), expand_rows, 'conv_igemm_b3', 'conv_igemm'),
                                                 (('b3',), gated_rows, 'conv_igemm_b3', 'conv_igemm')])


def test_mbconv_block_with_its_switches_off(dev, monkeypatch):
    from mydetection_amd import ops
    from mydetection_amd.external.efficientnet.model import BlockArgs, GlobalParams, MBConvBlock
    m = _module(MBConvBlock(BlockArgs(3, 1, CIN, COUT, 6, True, 1, 0.25), GlobalParams(0.99, 1e-3, 0.2, 1.0, 1.0, 8, 240)), dev)
    x = _input(dev)
    monkeypatch.setattr(ops, 'B3_GATED_MIN_COUT', 0)
    _run(monkeypatch, 'low', lambda: m(x), [(('b3',), 1, 'conv_igemm_b3', None), ((), 1, 'conv_igemm', None)])
    monkeypatch.setattr(ops, 'B3_EXPAND_MIN_ROWS', 0)
    _run(monkeypatch, 'shipped', lambda: m(x), [((), 0, None, 'conv_igemm'), ((), ops.B3_GATED_MIN_ROWS, None, 'conv_igemm')])


@pytest.mark.parametrize('thresholds', ['low', 'shipped'])
def test_yolo_head_prediction_conv(dev, monkeypatch, thresholds):
    """The head's 1x1 conv has the channel count its class gives it: 3 anchors x (4 + 1 + 80) = 255 on a pixel stride of 256."""
    from mydetection_amd import ops
    from mydetection_amd.models.rpns import YOLOHead
    m = _module(YOLOHead({'model.yolo.num_anchor_per_level': 3, 'general.num_class': 80, 'model.fpn.out_channels': [CIN]}), dev)
    x = _input(dev)
    preds = _run(monkeypatch, thresholds, lambda: m([x])[0].packed['box'][0], [(('b3',), None, 'conv_igemm_b3', 'conv_igemm')])
    assert preds.shape[1] == 255 and ops.nhwc_ld(preds) == 256


@pytest.mark.parametrize('thresholds', ['low', 'shipped'])
@pytest.mark.parametrize('cout,forms,low,shipped', [(COUT, ('wino', 'wino4'), 'conv_wino4', 'conv_wino'),
                                                   (81, ('wino', 'wino4'), 'conv_wino4', 'conv_wino'),
                                                   (4, (), 'conv_igemm', 'conv_igemm')])
def test_last_conv(dev, monkeypatch, thresholds, cout, forms, low, shipped):
    """The dense 3x3 last conv of a head branch: Winograd from 32 output channels up; 81 channels are computed as 84 with zero rows
    and returned as a view of them."""
    from mydetection_amd.models.rpns import _LastConv
    m = _module(_LastConv(88, cout, 3, 1, padding=1), dev)
    x = _input(dev, 88)
    y = _run(monkeypatch, thresholds, lambda: m(x), [(forms, None, low, shipped)], view_of_last=True)
    assert y.shape[1] == cout
