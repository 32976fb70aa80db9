"""Every feature-map kernel against float64 on tensors that pass 2^31 and 2^32 BYTES.

The rest of the suite runs tensors of a few megabytes (the largest: 1.68 GB); here every call has at least one tensor whose byte
offsets pass 2 GiB, most pass 4 GiB -- where 32-bit address arithmetic goes wrong without faulting: the conv kernels address memory
through buffer descriptors with 32-bit offsets (csrc/common.h: mydet_rsrc covers less than 2 GiB; loads past it return 0, stores are
dropped), every launcher has a window rule of its own to live with that, and the EfficientNet / BiFPN / resample / level-table kernels
use plain pointers whose offsets are widened by hand.  tests/_large.py holds the method: one run on the whole batch (the intended
kernel's ops.KernelTimer span), EVERY image compared on the device against the same call on chunks below 1 GiB, float64 on images 0,
B - 1 and the images around each crossing.  Images are all different (a seeded device generator).  Tolerances are the families' own:
FAMILY_TOL of tests/test_gpu_footprint.py and the bounds of the matching tests in tests/test_gpu_kernels.py / test_gpu_stem_p3.py /
test_gpu_lr_tb.py.  Shapes are the smallest at which each crossing exists; the kernel form is confirmed with the launcher's own host
rule before the launch.

Where each offset is widened or rebased, and which host rule bounds what stays 32-bit:

  conv_igemm / _b3 / upcat   x (and the half-size x1): descriptor rebased at the tile's first image b0, offsets bounded by
                             img_bytes * (256 / (Ho Wo) + 2) < 2^31 - 16;  y, residual: ONE descriptor, M * ld * 4 < 2^31 - 16
                             (MYDET_E_UNSUPP beyond);  gate [B][Cin]: one descriptor, B * Cin * 4 < 2^31 - 16 (guard added here)
  conv_wino / conv_wino4     x, y, residual: rebased at b0 (F(4x4)'s x one row + one pixel earlier), offsets bounded by
                             H W ldmax 4 (tiles / tiles-per-image + 2) < 2^31 - 16;  V workspace: 64-bit base per tile block,
                             offsets inside one block's nk * 18 432 bytes (bounded with U: 36 Cin CoutP 4 < 2^31 - 16)
  conv_p3 / conv_stem_p3     x (conv_p3), y, residual: descriptor per image, one image (+ a row and a pixel) <= 2^31 - 16
  pw_skinny, dwconv (three forms), channel_sums, mbconv_expand_dw, stem_dw, conv_stem, maxpool3s2, bifpn_fuse, upsample_concat,
  space_to_depth, spp_concat, sepconv_nodes, lr_tb_levels
                             plain pointers; the image / pixel index is int64 before it meets a stride (the loops count int64 items,
                             `(int64_t)b * H * W * ld`); grids: 1-D and bounded (< 2^31 workgroups, MYDET_E_UNSUPP) except the
                             squeeze forms' (S, B) grid, which needs B <= 65 535 (MYDET_E_BADARG)

Out of scope: tensors of 2^31 ELEMENTS or more (8 GiB), the uint8 frame / YUV / crop / draw entries, decode and post-process (bounded
per image by their own documented limits), and splitting an over-size batch on the host.
"""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from _arena import SENTINEL_BITS
from _large import EXACT, G31, G32, abs_tol, close_tol, rand_nchw, randn_nhwc, rel_tol, run_large
from _refs import act_f64, lr_tb_layer_f64, se_gate_f64, sepconv_node_f64
from test_gpu_footprint import FAMILY_SPAN, FAMILY_TOL

pytestmark = pytest.mark.gpu

E_UNSUPP = -2                                   # MYDET_E_UNSUPP of include/mydet.h


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    from mydetection_amd import _lib
    _lib.lib()                                   # fail loudly if the HIP library is missing
    return torch.device('cuda:0')


@pytest.fixture(autouse=True)
def _give_memory_back(dev):
    """Nothing of a multi-GiB test outlives it: the F(4x4) workspace and the squeeze-excite share buffer never shrink, and a later
    graph test would capture them."""
    from mydetection_amd import ops
    before = [t for d in (ops._WINO4_WS, ops._SE_SHARES) for t in d.values()]
    yield
    for d in (ops._WINO4_WS, ops._SE_SHARES):
        for k in [k for k, t in d.items() if k[:2] == (dev.type, dev.index) and not any(t is b for b in before)]:
            d.pop(k)                                # (as tests/test_host_cpu.py does: the next user sizes its own)
    del before
    torch.cuda.empty_cache()


def _gen(dev, seed):
    return torch.Generator(device=dev).manual_seed(seed)


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


# --------------------------------------------------------------------------------------------------------------- convolutions
def _conv_large(dev, fam, *, B, Cin, Cout, k, s, H, W, act, residual=False, gate=False, ldy=None, ldr=None, crossing=True, extra_named=None):
    """One conv family on a large batch.  fam: igemm b3 wino wino4 p3 (FAMILY_SPAN / FAMILY_TOL)."""
    from mydetection_amd import _lib, ops
    pad = ((k - 1) // 2,) * 4
    Ho, Wo = ops.conv_out_size(H, k, s, pad[0], pad[2]), ops.conv_out_size(W, k, s, pad[1], pad[3])
    g = _gen(dev, 7 * Cin + Cout + k + s)
    w = torch.randn(Cout, Cin, k, k, generator=g, device=dev) / (Cin * k * k) ** 0.5
    scale, shift = torch.rand(Cout, generator=g, device=dev) + 0.5, torch.randn(Cout, generator=g, device=dev) * 0.1
    wd = w.permute(0, 2, 3, 1).contiguous()
    u = ops.wino_weights(wd) if fam == 'wino' else None
    u4 = ops.wino4_weights(wd) if fam == 'wino4' else None
    w3 = ops.split_bf16(wd) if fam in ('b3', 'p3') else None
    M = B * Ho * Wo
    ldx, ldyy, ldrr = Cin, ldy or Cout, (ldr or Cout) if residual else 0
    out = (ctypes.c_int32 * 16)()
    # ---- the launcher's own host rule says which kernel this is
    if fam in ('igemm', 'b3'):
        assert ops.conv_size_refusals('igemm', B, H, W, Ho, Wo, ldx, ldyy, ldrr) == []
        assert not (k == 1 and Cout <= 48 and M >= 65536), 'this shape goes to the skinny pointwise kernel'
    if fam == 'igemm':
        _lib.check(_lib.lib().mydet_conv_igemm_plan(-1, B, Ho, Wo, Cin, Cout, k * k, ops.WORKSPACE_BYTES, _cus(), out), 'mydet_conv_igemm_plan')
    if fam == 'b3':
        assert w3 is not None and ops.b3_takes(M, Cin, Cout, k, 1, min_cout=ops.B3_GATED_MIN_COUT if gate else 128)
        assert not gate or (k == 1 and act == ops.ACT_NONE)
    if fam == 'wino':
        assert u is not None and ops.WINOGRAD and ops.conv_size_refusals('wino', B, H, W, Ho, Wo, ldx, ldyy, ldrr) == []
        _lib.check(_lib.lib().mydet_wino_plan(B, H, W, Cin, Cout, ops.WORKSPACE_BYTES, _cus(), out), 'mydet_wino_plan')
    if fam == 'wino4':
        assert u4 is not None and ops.WINOGRAD and ops.WINOGRAD4 and ops.conv_size_refusals('wino4', B, H, W, Ho, Wo, ldx, ldyy, ldrr) == []
        assert _lib.lib().mydet_wino4_tail_plan(B, H, W, Cin, Cout, 2 * _cus(), ctypes.cast(out, ctypes.c_void_p)) >= 0
    if fam == 'p3':
        assert w3 is not None and ops.CONV_P3 and ops.p3_takes(B, Ho, Wo, Cin, Cout, k, s, pad) and ops.p3_plan(Ho, Wo, Cout, s).tiles_img > 0
    batched = dict(x=randn_nhwc(g, B, Cin, H, W))
    if residual:
        batched['res'] = randn_nhwc(g, B, Cout, Ho, Wo, ld=ldr)
    if gate:
        batched['gate'] = torch.rand(B, Cin, generator=g, device=dev)

    def call(x, res=None, gate=None):
        p3_was = ops.CONV_P3
        ops.CONV_P3 = fam == 'p3'
        try:
            if fam == 'p3':
                assert ops.p3_takes(x.shape[0], Ho, Wo, Cin, Cout, k, s, pad)
            return ops.conv2d(x, wd, scale, shift, k, s, pad, act, residual=res, gate=gate, out_ld=ldy, wino=u, wino4=u4, b3=w3,
                              b3_min_rows=1 if fam == 'b3' else None)
        finally:
            ops.CONV_P3 = p3_was

    wc, sc, sh = w.cpu().double(), scale.cpu().double().view(1, -1, 1, 1), shift.cpu().double().view(1, -1, 1, 1)

    def ref64(x, res=None, gate=None):
        if gate is not None:
            x = x * gate.view(-1, Cin, 1, 1)
        r = act_f64(F.conv2d(F.pad(x, (pad[1], pad[3], pad[0], pad[2])), wc, None, s) * sc + sh, act)
        return r + res if res is not None else r

    rel, floor1 = FAMILY_TOL[fam]
    named = extra_named(B) if extra_named else ()
    return run_large(dev, f'{FAMILY_SPAN[fam]} {Cin}->{Cout} k{k}s{s} {H}x{W}' + (' +res' if residual else '') + (' gated' if gate else ''), call,
                     batched, [rel_tol(rel, floor1)], ref64, span=FAMILY_SPAN[fam], exact=fam == 'p3', extra_named=named, crossing=crossing)


@pytest.mark.parametrize('fam,case', [
    # x 4 MiB / image = 4160 MiB (2^31 inside image 512, 2^32 at image 1024); y and residual 1040 MiB
    ('igemm', dict(B=1040, Cin=256, Cout=64, k=1, s=1, H=64, W=64, act=1, residual=True)),
    ('b3', dict(B=1040, Cin=256, Cout=64, k=1, s=1, H=64, W=64, act=0, residual=True, gate=True)),
    # the same bytes behind a 3x3 stride-2 window: halo rows and the b0 window at both crossings
    ('igemm', dict(B=1040, Cin=64, Cout=64, k=3, s=2, H=128, W=128, act=1, residual=True)),
    ('b3', dict(B=1040, Cin=64, Cout=64, k=3, s=2, H=128, W=128, act=0, residual=True)),
], ids=['igemm-1x1', 'b3-1x1-gated', 'igemm-3x3s2', 'b3-3x3s2'])
def test_large_conv_igemm(dev, fam, case):
    _conv_large(dev, fam, **case)


@pytest.mark.parametrize('case', [
    dict(B=8200, Cin=32, Cout=32, k=3, s=1, H=64, W=64, act=1),                       # x, y 512 KiB / image = 4100 MiB
    dict(B=4112, Cin=32, Cout=32, k=3, s=1, H=64, W=64, act=1, residual=True),        # x, y, residual 2056 MiB
], ids=['plain', 'residual'])
def test_large_conv_wino(dev, case):
    _conv_large(dev, 'wino', **case)


@pytest.mark.parametrize('residual', [False, True], ids=['plain', 'residual'])
def test_large_conv_wino4(dev, residual):
    """x, y (residual) 2056 MiB; the transform-domain workspace V passes 2^32: its crossings name images too."""
    from mydetection_amd import _lib
    B, Cin, Cout, H, W = 4112, 32, 32, 64, 64
    nbytes = lambda b: int(_lib.lib().mydet_wino4_workspace_bytes(b, H, W, Cin, Cout))      # noqa: E731
    while nbytes(B) <= G32:
        B += 16
    print(f'F(4x4) workspace of B = {B}: {nbytes(B)} bytes = {nbytes(B) / 2 ** 20:.0f} MiB ({nbytes(B) / (B * H * W * Cin * 4):.3f} x the input)')
    block, tpi = (Cin >> 2) * 18432, ((H + 3) // 4) * ((W + 3) // 4)          # bytes of V per block of 32 tiles (csrc/conv_wino4.hip: V_BYTES)

    def v_crossings(b):
        imgs = {beta // block * 32 // tpi for beta in (G31, G32)}
        return {i + d for i in imgs for d in (-1, 0, 1)}

    _conv_large(dev, 'wino4', B=B, Cin=Cin, Cout=Cout, k=3, s=1, H=H, W=W, act=1, residual=residual, extra_named=v_crossings)


@pytest.mark.parametrize('case', [
    dict(B=4112, Cin=16, Cout=64, k=3, s=1, H=64, W=64, act=1, residual=True),        # y, residual 1 MiB / image = 4112 MiB
    dict(B=1040, Cin=64, Cout=64, k=3, s=2, H=128, W=128, act=1),                     # x 4 MiB / image = 4160 MiB
], ids=['s1-residual', 's2'])
def test_large_conv_p3(dev, case):
    _conv_large(dev, 'p3', **case)


def test_large_conv1x1_upcat(dev):
    """The smallest (C_lo, C_hi, Cout) the fused launch accepts with hi > 2^32 and y < 2^31: the 64 x 64 x 32 tile needs Cout > 64 and
    channel counts % 32, so y < hi / 2 needs C_hi >= 160 at Cout = 68: hi 160 KiB / image = 4219 MiB, y 1793 MiB, lo 211 MiB (the img1
    window of the half-size map moves with b0 as well)."""
    from mydetection_amd import ops
    B, C_lo, C_hi, Cout, H, W = 27000, 32, 160, 68, 16, 16
    g = _gen(dev, 5)
    w = torch.randn(Cout, C_lo + C_hi, 1, 1, generator=g, device=dev) / (C_lo + C_hi) ** 0.5
    scale, shift = torch.rand(Cout, generator=g, device=dev) + 0.5, torch.randn(Cout, generator=g, device=dev) * 0.1
    wd = w.permute(0, 2, 3, 1).contiguous()
    batched = dict(lo=randn_nhwc(g, B, C_lo, H // 2, W // 2), hi=randn_nhwc(g, B, C_hi, H, W))
    assert B * H * W * C_hi * 4 > G32 and B * H * W * Cout * 4 < G31

    def call(lo, hi):
        y = ops.conv1x1_upcat(lo, hi, wd, scale, shift, ops.ACT_LEAKY)
        assert y is not None, 'the fused launch refused the shape'
        return y

    wc, sc, sh = w.cpu().double(), scale.cpu().double().view(1, -1, 1, 1), shift.cpu().double().view(1, -1, 1, 1)

    def ref64(lo, hi):
        return act_f64(F.conv2d(torch.cat((F.interpolate(lo, scale_factor=(2, 2), mode='nearest'), hi), 1), wc) * sc + sh, 1)

    run_large(dev, f'conv1x1_upcat {C_lo}^+{C_hi}->{Cout}', call, batched, [rel_tol(*FAMILY_TOL['igemm'])], ref64, span='conv_igemm', exact=False)


def test_large_pw_skinny(dev):
    """240 -> 40 at 64 x 64 with gate and residual, through mydet_conv2d_igemm_f32: x 3.75 MiB / image = 4125 MiB."""
    from mydetection_amd import ops
    B, Cin, Cout, H, W = 1100, 240, 40, 64, 64
    assert Cout <= 48 and B * H * W >= 65536 and H * W >= 512 and Cin <= 240             # mydet_conv2d_igemm_f32's and mydet_pw_skinny's rule
    g = _gen(dev, 6)
    w = torch.randn(Cout, Cin, 1, 1, generator=g, device=dev) / Cin ** 0.5
    scale, shift = torch.rand(Cout, generator=g, device=dev) + 0.5, torch.randn(Cout, generator=g, device=dev) * 0.1
    wd = w.permute(0, 2, 3, 1).contiguous()
    batched = dict(x=randn_nhwc(g, B, Cin, H, W), res=randn_nhwc(g, B, Cout, H, W), gate=torch.rand(B, Cin, generator=g, device=dev))
    wc, sc, sh = w.cpu().double(), scale.cpu().double().view(1, -1, 1, 1), shift.cpu().double().view(1, -1, 1, 1)
    def call(x, res, gate):
        assert x.shape[0] * H * W >= 65536, 'a chunk this small leaves the skinny kernel'
        return ops.conv2d(x, wd, scale, shift, 1, 1, (0, 0, 0, 0), 0, residual=res, gate=gate)

    run_large(dev, 'pw_skinny 240->40 gated +res', call, batched, [rel_tol(2e-5, True)],
              lambda x, res, gate: F.conv2d(x * gate.view(-1, Cin, 1, 1), wc) * sc + sh + res, span='conv_igemm', exact=True)


# ----------------------------------------------------------------------------------------------------------------- the stems
def _stem_operands(dev, g):
    w = torch.randn(32, 3, 3, 3, generator=g, device=dev) * 0.2
    scale, shift = torch.rand(32, generator=g, device=dev) + 0.5, torch.randn(32, generator=g, device=dev) * 0.1
    return w, scale, shift


def test_large_conv_stem(dev):
    """Image [B,3,64,64], stride 2: the 32-channel 32 x 32 output is 128 KiB / image = 4100 MiB."""
    from mydetection_amd import ops
    B, pad = 32800, (0, 0, 1, 1)
    g = _gen(dev, 11)
    w, scale, shift = _stem_operands(dev, g)
    wd = w.permute(0, 2, 3, 1).contiguous()
    wc, sc, sh = w.cpu().double(), scale.cpu().double().view(1, -1, 1, 1), shift.cpu().double().view(1, -1, 1, 1)
    run_large(dev, 'conv_stem s2', lambda x: ops.conv2d_stem(x, wd, scale, shift, 2, pad, ops.ACT_LEAKY), dict(x=rand_nchw(g, B, 3, 64, 64)),
              [abs_tol(1e-5)], lambda x: act_f64(F.conv2d(F.pad(x, (pad[1], pad[3], pad[0], pad[2])), wc, None, 2) * sc + sh, 1),
              span='conv_stem', exact=True)


def test_large_conv_stem_p3(dev):
    """Image [B,3,64,64] -> the fused stem + stride-2 conv: 64-channel 32 x 32 output, 256 KiB / image = 8200 MiB."""
    from mydetection_amd import ops
    B, Cout = 32800, 64
    g = _gen(dev, 12)
    w0 = torch.randn(32, 3, 3, 3, generator=g, device=dev) / 27 ** 0.5
    sc0, sh0 = torch.rand(32, generator=g, device=dev) + 0.5, torch.rand(32, generator=g, device=dev) * 0.4 + 0.1
    w1 = torch.randn(Cout, 32, 3, 3, generator=g, device=dev) / 288 ** 0.5
    sc1, sh1 = torch.rand(Cout, generator=g, device=dev) + 0.5, torch.randn(Cout, generator=g, device=dev) * 0.1
    w0p, w1p = ops.stem_p3_weights(w0.permute(0, 2, 3, 1).contiguous()), ops.split_bf16(w1.permute(0, 2, 3, 1).contiguous())
    assert ops.stem_p3_takes(B, 64, 64, Cout, (1, 1, 1, 1))

    def call(x):
        y = ops.conv_stem_p3(x, w0p, sc0, sh0, (1, 1, 1, 1), w1p, sc1, sh1)
        assert y is not None
        return y

    c = lambda t: t.cpu().double()                          # noqa: E731

    def ref64(x):
        mid = F.leaky_relu(F.conv2d(F.pad(x, (1, 1, 1, 1)), c(w0)) * c(sc0).view(1, -1, 1, 1) + c(sh0).view(1, -1, 1, 1), 0.1)
        return F.leaky_relu(F.conv2d(F.pad(mid, (1, 1, 1, 1)), c(w1), None, 2) * c(sc1).view(1, -1, 1, 1) + c(sh1).view(1, -1, 1, 1), 0.1)

    run_large(dev, 'conv_stem_p3', call, dict(x=rand_nchw(g, B, 3, 64, 64)), [rel_tol(2e-5, False)], ref64, span='conv_stem_p3', exact=True)


def test_large_stem_dw(dev):
    """Image [B,3,64,64] -> EfficientNet stem + depthwise: 32-channel 32 x 32 output 4100 MiB, and its per-tile channel sums."""
    from mydetection_amd import ops
    B, pad = 32800, (0, 0, 1, 1)
    g = _gen(dev, 13)
    ws, wdw = torch.randn(32, 3, 3, 3, generator=g, device=dev) * 0.3, torch.randn(32, 1, 3, 3, generator=g, device=dev) * 0.3
    sc0, sh0 = torch.rand(32, generator=g, device=dev) + 0.5, torch.randn(32, generator=g, device=dev) * 0.2
    sc1, sh1 = torch.rand(32, generator=g, device=dev) + 0.5, torch.randn(32, generator=g, device=dev) * 0.2
    ws_o, wd_k = ws.permute(0, 2, 3, 1).contiguous(), wdw.permute(2, 3, 0, 1).reshape(3, 3, 32).contiguous()
    args = (ops.fold_scale(ws_o, sc0), sh0, ops.fold_scale(wd_k, sc1), sh1)

    def call(x):
        y, partial = ops.stem_dw(x, *args, pad)
        return y, partial[:, :-1]

    c = lambda t: t.cpu().double()                          # noqa: E731

    def ref64(x):
        t = F.conv2d(F.pad(x, (pad[1], pad[3], pad[0], pad[2])), c(ws), stride=2) * c(sc0).view(1, -1, 1, 1) + c(sh0).view(1, -1, 1, 1)
        t = t * torch.sigmoid(t)
        r = F.conv2d(t, c(wdw), padding=1, groups=32) * c(sc1).view(1, -1, 1, 1) + c(sh1).view(1, -1, 1, 1)
        r = r * torch.sigmoid(r)
        return r, r.sum(dim=(2, 3))

    run_large(dev, 'stem_dw', call, dict(x=rand_nchw(g, B, 3, 64, 64, -1.0, 1.0)), [rel_tol(3e-5, True), close_tol(1e-5, 1e-3)], ref64,
              span='stem_dw', exact=True, reduce=[None, lambda p: p.sum(dim=1)])


def test_large_space_to_depth(dev):
    """Image [B,3,64,64] -> [B,12,32,32]: pure data movement, image and output read / written past 2^31 bytes at B = 49200."""
    from mydetection_amd import ops
    B = 49200                                               # the 12-channel output is 48 KiB / image: 2306 MiB (B = 32800 of the stems: 1537 MiB, no crossing)
    g = _gen(dev, 14)
    run_large(dev, 'space_to_depth', ops.space_to_depth, dict(x=rand_nchw(g, B, 3, 64, 64)), [EXACT],
              lambda x: torch.cat([x[..., ::2, ::2], x[..., 1::2, ::2], x[..., ::2, 1::2], x[..., 1::2, 1::2]], 1), span='space_to_depth', exact=True)


# ------------------------------------------------------------------------------------------------- EfficientNet family kernels
def _dw_operands(dev, g, C, k):
    w = torch.randn(C, 1, k, k, generator=g, device=dev) * 0.3
    scale, shift = torch.rand(C, generator=g, device=dev) + 0.5, torch.randn(C, generator=g, device=dev) * 0.1
    return w, w.permute(2, 3, 0, 1).reshape(k, k, C).contiguous(), scale, shift


def _dw_ref(w, scale, shift, k, s, pad, C):
    wc, sc, sh = w.cpu().double(), scale.cpu().double().view(1, -1, 1, 1), shift.cpu().double().view(1, -1, 1, 1)
    return lambda x: act_f64(F.conv2d(F.pad(x, (pad[1], pad[3], pad[0], pad[2])), wc, None, s, 0, 1, C) * sc + sh, 2)


DW_FORMS = {'tiled-wide': dict(k=3, s=1, C=32, B=8200, pad=(1, 1, 1, 1)),          # LDS-tiled, 8 quads x (8 x 16): x and y 4100 MiB
            'tiled-narrow': dict(k=5, s=1, C=16, B=16400, pad=(2, 2, 2, 2)),       # LDS-tiled, 4 quads x (8 x 32)
            'register-blocked': dict(k=3, s=2, C=32, B=8200, pad=(0, 0, 1, 1))}    # stride 2: x 4100 MiB, y 1025 MiB


@pytest.mark.parametrize('squeeze', [False, True], ids=['plain', 'squeeze'])
@pytest.mark.parametrize('form', list(DW_FORMS))
def test_large_dwconv(dev, form, squeeze):
    from mydetection_amd import _lib, ops
    f = DW_FORMS[form]
    k, s, C, B, pad = f['k'], f['s'], f['C'], f['B'], f['pad']
    Ho = ops.conv_out_size(64, k, s, pad[0], pad[2])
    tiles = ((Ho + 7) // 8) * ((Ho + 15) // 16 if C >= 32 else (Ho + 31) // 32)
    # mydet_dwconv_slices is the launcher's own rule: one slice per tile says "LDS-tiled", min(128, pixels / 16) the register-blocked form
    assert _lib.lib().mydet_dwconv_slices(Ho, Ho, C, k, s) == (tiles if s == 1 else min(128, Ho * Ho // 16))
    g = _gen(dev, 20 + k + s + C)
    w, wk, scale, shift = _dw_operands(dev, g, C, k)
    ref = _dw_ref(w, scale, shift, k, s, pad, C)
    if squeeze:
        def call(x):
            y, partial = ops.dwconv(x, wk, scale, shift, k, s, pad, ops.ACT_SWISH, squeeze=True)
            return y, partial[:, :-1]
        run_large(dev, f'dwconv {form} squeeze', call, dict(x=randn_nhwc(g, B, C, 64, 64)), [abs_tol(2e-5), close_tol(1e-5, 1e-4)],
                  lambda x: (ref(x), ref(x).sum(dim=(2, 3))), span='dwconv', exact=True, reduce=[None, lambda p: p.sum(dim=1)])
    else:
        run_large(dev, f'dwconv {form}', lambda x: ops.dwconv(x, wk, scale, shift, k, s, pad, ops.ACT_SWISH), dict(x=randn_nhwc(g, B, C, 64, 64)),
                  [abs_tol(2e-5)], ref, span='dwconv', exact=True)


def test_large_dwconv_se_tail(dev):
    """The register-blocked form with the squeeze-excite gate finished inside the launch: 8200 images' shares in one share buffer."""
    from mydetection_amd import ops
    f = DW_FORMS['register-blocked']
    k, s, C, B, pad, Cse = f['k'], f['s'], f['C'], f['B'], f['pad'], 8
    g = _gen(dev, 31)
    w, wk, scale, shift = _dw_operands(dev, g, C, k)
    w1, b1 = torch.randn(Cse, C, generator=g, device=dev) * 0.1, torch.randn(Cse, generator=g, device=dev) * 0.1
    w2t, b2 = torch.randn(Cse, C, generator=g, device=dev) * 0.3, torch.randn(C, generator=g, device=dev) * 0.1
    ref = _dw_ref(w, scale, shift, k, s, pad, C)
    c = lambda t: t.cpu().double()                          # noqa: E731
    run_large(dev, 'dwconv register-blocked + SE tail', lambda x: ops.dwconv(x, wk, scale, shift, k, s, pad, ops.ACT_SWISH, se=(w1, b1, w2t, b2)),
              dict(x=randn_nhwc(g, B, C, 64, 64)), [abs_tol(2e-5), abs_tol(1e-5)], lambda x: (ref(x), se_gate_f64(ref(x), c(w1), c(b1), c(w2t), c(b2))),
              span='dwconv', exact=True)
    assert ops.se_tail_timeouts(dev) == 0


def test_large_mbconv_expand_dw(dev):
    """Cin 24 (Cexp 144), k3 s1, 32 x 64: y 1152 KiB / image = 4106 MiB at B = 3650."""
    from mydetection_amd import ops
    B, cin, k, s, H, W, pad = 3650, 24, 3, 1, 32, 64, (1, 1, 1, 1)
    cexp = 6 * cin
    assert (k, s, cin) in ops.MBCONV_FUSED_SHAPES
    g = _gen(dev, 41)
    we = torch.randn(cexp, cin, generator=g, device=dev) / cin ** 0.5
    wdw = torch.randn(k, k, cexp, generator=g, device=dev) / k
    sc0, sh0 = torch.rand(cexp, generator=g, device=dev) + 0.5, torch.randn(cexp, generator=g, device=dev) * 0.3
    sc1, sh1 = torch.rand(cexp, generator=g, device=dev) + 0.5, torch.randn(cexp, generator=g, device=dev) * 0.3
    args = (ops.fold_scale(we.view(cexp, 1, 1, cin).contiguous(), sc0), sh0, ops.fold_scale(wdw, sc1), sh1)

    def call(x):
        y, partial = ops.mbconv_expand_dw(x, *args, k, s, pad)
        return y, partial[:, :-1]

    c = lambda t: t.cpu().double()                          # noqa: E731

    def ref64(x):
        e = F.conv2d(x, c(we).view(cexp, cin, 1, 1)) * c(sc0).view(1, -1, 1, 1) + c(sh0).view(1, -1, 1, 1)
        e = F.pad(e * torch.sigmoid(e), (pad[1], pad[3], pad[0], pad[2]))
        y = F.conv2d(e, c(wdw).permute(2, 0, 1).reshape(cexp, 1, k, k), None, s, 0, 1, cexp) * c(sc1).view(1, -1, 1, 1) + c(sh1).view(1, -1, 1, 1)
        y = y * torch.sigmoid(y)
        return y, y.sum(dim=(2, 3))

    run_large(dev, 'mbconv_expand_dw 24->144 k3s1', call, dict(x=randn_nhwc(g, B, cin, H, W)), [rel_tol(2e-5, True), close_tol(1e-4, 1e-3)], ref64,
              span='mbconv_expand_dw', exact=True, reduce=[None, lambda p: p.sum(dim=1)])


def test_large_maxpool_channel_sums(dev):
    """C = 32, 64 x 64, B = 8200: x 4100 MiB through the max pool and through the standalone squeeze."""
    from mydetection_amd import ops
    B, C = 8200, 32
    g = _gen(dev, 51)
    x = randn_nhwc(g, B, C, 64, 64)
    run_large(dev, 'maxpool3s2', ops.maxpool3s2, dict(x=x), [EXACT], lambda x: F.max_pool2d(x, 3, 2, 1), span='maxpool', exact=True)
    run_large(dev, 'channel_sums', lambda x: ops.channel_sums(x)[:, :-1], dict(x=x), [close_tol(1e-5, 1e-4)], lambda x: x.sum(dim=(2, 3)),
              span=None, exact=True, reduce=[lambda p: p.sum(dim=1)])


@pytest.mark.parametrize('mode', ['up2x', 'pool'])
def test_large_bifpn_fuse(dev, mode):
    """Two inputs, each mode once; the 32-channel 64 x 64 map (4100 MiB at B = 8200) is the same-size input of the up-sampling node and
    the pooled input of the down-sampling node (its 128 x 128 partner would be 16 GiB)."""
    from mydetection_amd import ops
    B, C = 8200, 32
    g = _gen(dev, 52)
    big, small = randn_nhwc(g, B, C, 64, 64), randn_nhwc(g, B, C, 32, 32)
    wts = torch.tensor([0.7, 1.2], device=dev)
    wn = F.relu(wts.cpu().double())
    wn = wn / (wn.sum() + 0.0001)
    swish = lambda t: t * torch.sigmoid(t)                  # noqa: E731
    if mode == 'up2x':
        run_large(dev, 'bifpn_fuse same + up2x', lambda a, b: ops.bifpn_fuse([a, b], [ops.FUSE_SAME, ops.FUSE_UP2X], wts), dict(a=big, b=small),
                  [close_tol(2e-6, 1e-7)], lambda a, b: swish(wn[0] * a + wn[1] * F.interpolate(b, scale_factor=(2, 2), mode='nearest')),
                  span='bifpn_fuse', exact=True)
    else:
        run_large(dev, 'bifpn_fuse same + pool', lambda a, b: ops.bifpn_fuse([a, b], [ops.FUSE_SAME, ops.FUSE_POOL], wts), dict(a=small, b=big),
                  [close_tol(2e-6, 1e-7)], lambda a, b: swish(wn[0] * a + wn[1] * F.max_pool2d(b, 3, 2, 1)), span='bifpn_fuse', exact=True)


def test_large_upsample_concat(dev):
    """lo C = 32 at 32 x 32, hi C = 32 at 64 x 64, B = 4112: y 4112 MiB, hi 2056 MiB."""
    from mydetection_amd import ops
    B = 4112
    g = _gen(dev, 53)
    run_large(dev, 'upsample_concat', lambda a, b: ops.upsample_concat(a, (64, 64), b), dict(a=randn_nhwc(g, B, 32, 32, 32), b=randn_nhwc(g, B, 32, 64, 64)),
              [EXACT], lambda a, b: torch.cat((F.interpolate(a, size=(64, 64), mode='nearest'), b), 1), span='upsample_concat', exact=True)


def test_large_spp_concat(dev):
    """C = 32 at 20 x 20, B = 21000: y 200 KiB / image = 4101 MiB."""
    from mydetection_amd import ops
    g = _gen(dev, 54)
    run_large(dev, 'spp_concat', ops.spp_concat, dict(x=randn_nhwc(g, 21000, 32, 20, 20)), [EXACT],
              lambda x: torch.cat([x] + [F.max_pool2d(x, k, 1, k // 2) for k in (5, 9, 13)], 1), span='spp_concat', exact=True)


def test_large_sepconv_nodes(dev):
    """C = 88 at 16 x 16, B = 48000 (88 KiB / image = 4125 MiB in and out): one identity node and one two-input node in one launch."""
    from mydetection_amd import ops
    B, C = 48000, 88
    g = _gen(dev, 61)

    def weights(bn):
        return dict(w_dw=torch.randn(3, 3, C, generator=g, device=dev) / 3.0, w_pw=torch.randn(C, C, generator=g, device=dev) / C ** 0.5,
                    scale=torch.rand(C, generator=g, device=dev) + 0.5 if bn else None, shift=torch.randn(C, generator=g, device=dev) * 0.2)

    n0, n1 = weights(True), weights(True)
    fw = torch.tensor([0.8, 1.3], device=dev)
    packed = [ops.pack_pointwise(n['w_pw']) for n in (n0, n1)]

    def call(a, b, h):
        return ops.sepconv_nodes([dict(inputs=[a], modes=[0], w_dw=n0['w_dw'], w_pw=packed[0], scale=n0['scale'], shift=n0['shift'], cout=C, act=2),
                                  dict(inputs=[b, h], modes=[0, 1], fuse_weights=fw, w_dw=n1['w_dw'], w_pw=packed[1], scale=n1['scale'],
                                       shift=n1['shift'], cout=C, act=0)])

    c = lambda t: None if t is None else t.cpu()            # noqa: E731

    def ref64(a, b, h):
        return (sepconv_node_f64([a], [0], None, c(n0['w_dw']), c(n0['w_pw']), c(n0['scale']), c(n0['shift']), 2),
                sepconv_node_f64([b, h], [0, 1], c(fw), c(n1['w_dw']), c(n1['w_pw']), c(n1['scale']), c(n1['shift']), 0))

    run_large(dev, 'sepconv_nodes', call, dict(a=randn_nhwc(g, B, C, 16, 16), b=randn_nhwc(g, B, C, 16, 16), h=randn_nhwc(g, B, C, 8, 8)),
              [rel_tol(2e-5, True), rel_tol(2e-5, True)], ref64, span='sepconv_nodes', exact=True)


def test_large_lr_tb_levels(dev):
    """C = 88 at 16 x 16, B = 48000: x 4125 MiB."""
    from mydetection_amd import ops
    B, C = 48000, 88
    g = _gen(dev, 62)
    ws = [torch.randn(C, 1, 3, 3, generator=g, device=dev), torch.randn(C, 1, 3, 3, generator=g, device=dev), torch.randn(2, C, 1, 3, generator=g, device=dev) * 0.3,
          torch.randn(2, generator=g, device=dev), torch.randn(2, C, 3, 1, generator=g, device=dev) * 0.3, torch.randn(2, generator=g, device=dev)]
    lr0, tb0, lr1, blr, tb1, btb = ws
    packed = ops.pack_lr_tb(lr0, tb0, lr1, blr, tb1, btb)
    cw = [t.cpu() for t in (lr0, tb0, lr1, blr, tb1, btb)]
    rms_tol = lambda ref: 1e-5 * float((ref ** 2).mean().sqrt())        # noqa: E731  (tests/test_gpu_lr_tb.py: _close)
    run_large(dev, 'lr_tb_levels', lambda x: ops.lr_tb_levels([(x, packed)])[0], dict(x=randn_nhwc(g, B, C, 16, 16)), [rms_tol],
              lambda x: lr_tb_layer_f64(x, *cw), span='lr_tb', exact=True)


# ------------------------------------------------------------------------------------------------------------------- guards
def _igemm_entries(dev, x, w, w3, res, ldr, y, ldy, B, H, W, Cin, Cout):
    """Return codes of both direct-conv C entries for a 1x1 layer, called as ops.conv2d calls them."""
    from mydetection_amd import _lib, ops
    ws = ops.conv_workspace(dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)      # noqa: E731
    tail = (p(ws), ws.numel() * 4, p(y), ldy, B, H, W, Cin, Cout, 1, 1, 1, 0, 0, H, W, 0, ops._stream())
    rc32 = _lib.lib().mydet_conv2d_igemm_f32(p(x), Cin, p(w), None, None, p(res), ldr, None, *tail)
    rcb3 = _lib.lib().mydet_conv2d_igemm_b3_f32(p(x), Cin, p(w3), None, None, p(res), ldr, None, *tail)
    torch.cuda.synchronize()
    return rc32, rcb3


def _untouched(t):
    return not bool((t.view(torch.int32) != SENTINEL_BITS).any())


def test_guard_igemm_output_below_2gib(dev):
    """1x1, 16 -> 64 at 64 x 64: B = 2047 (y = 2^31 - 2^20 bytes) runs and is right; B = 2048 (y = 2^31) is refused by both entries,
    ops.conv2d raises with the limit and the size, and no word of y changes."""
    from mydetection_amd import _lib, ops
    Cin, Cout, H, W = 16, 64, 64, 64
    _conv_large(dev, 'igemm', B=2047, Cin=Cin, Cout=Cout, k=1, s=1, H=H, W=W, act=1, crossing=False)
    _conv_large(dev, 'b3', B=2047, Cin=Cin, Cout=Cout, k=1, s=1, H=H, W=W, act=0, gate=True, crossing=False)
    torch.cuda.empty_cache()
    B = 2048
    g = _gen(dev, 71)
    x = randn_nhwc(g, B, Cin, H, W)
    wd = torch.randn(Cout, 1, 1, Cin, generator=g, device=dev)
    buf = torch.full((B, H, W, Cout), SENTINEL_BITS, dtype=torch.int32, device=dev).view(torch.float32)
    assert buf.numel() * 4 == G31
    assert _igemm_entries(dev, x, wd, ops.split_bf16(wd), None, 0, buf, Cout, B, H, W, Cin, Cout) == (E_UNSUPP, E_UNSUPP)
    assert _untouched(buf)
    with pytest.raises(_lib.MydetError) as e:
        ops.conv2d(x, wd, None, None, 1, 1, (0, 0, 0, 0), 0, out=buf.permute(0, 3, 1, 2))
    msg = str(e.value)
    assert 'mydet_conv2d_igemm_f32 failed: unsupported configuration' in msg and 'output' in msg and str(G31) in msg and str(ops.CONV_OFFSET_LIMIT) in msg
    assert _untouched(buf)


def test_guard_igemm_residual_below_2gib(dev):
    """The same pair for the residual rule, y narrower than the residual: 16 -> 52 channels, the residual a 52-channel slice of a
    64-wide buffer (B = 2048: its pixels span 2^31 bytes; y is 1.6 GiB)."""
    from mydetection_amd import _lib, ops
    Cin, Cout, H, W, ldr = 16, 52, 64, 64, 64
    _conv_large(dev, 'igemm', B=2047, Cin=Cin, Cout=Cout, k=1, s=1, H=H, W=W, act=1, residual=True, ldr=ldr, crossing=False)
    torch.cuda.empty_cache()
    B = 2048
    g = _gen(dev, 72)
    x, res = randn_nhwc(g, B, Cin, H, W), randn_nhwc(g, B, Cout, H, W, ld=ldr)
    wd = torch.randn(Cout, 1, 1, Cin, generator=g, device=dev)
    buf = torch.full((B, H, W, Cout), SENTINEL_BITS, dtype=torch.int32, device=dev).view(torch.float32)
    assert B * H * W * ldr * 4 == G31 and buf.numel() * 4 < G31
    assert _igemm_entries(dev, x, wd, ops.split_bf16(wd), res, ldr, buf, Cout, B, H, W, Cin, Cout) == (E_UNSUPP, E_UNSUPP)
    assert _untouched(buf)
    with pytest.raises(_lib.MydetError, match=f'residual: {G31} bytes'):
        ops.conv2d(x, wd, None, None, 1, 1, (0, 0, 0, 0), 0, residual=res, out=buf.permute(0, 3, 1, 2))
    assert _untouched(buf)


def test_guard_igemm_gate_below_2gib(dev):
    """gate [B][Cin] is read through one descriptor: B * Cin * 4 = 2^31 (1 x 1 maps, Cin = 64, B = 2^23) is refused by both entries and
    leaves y alone; B = 2^23 - 1 runs and is right."""
    from mydetection_amd import _lib, ops
    Cin, Cout = 64, 52                               # (52 outputs: not the skinny pointwise kernel's shape, and y stays below 2 GiB)
    _conv_large(dev, 'igemm', B=(1 << 23) - 1, Cin=Cin, Cout=Cout, k=1, s=1, H=1, W=1, act=0, gate=True, crossing=False)
    torch.cuda.empty_cache()
    B = 1 << 23
    g = _gen(dev, 73)
    x, gate = randn_nhwc(g, B, Cin, 1, 1), torch.rand(B, Cin, generator=g, device=dev)
    wd = torch.randn(Cout, 1, 1, Cin, generator=g, device=dev)
    buf = torch.full((B, 1, 1, Cout), SENTINEL_BITS, dtype=torch.int32, device=dev).view(torch.float32)
    ws = ops.conv_workspace(dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())             # noqa: E731
    tail = (p(gate), p(ws), ws.numel() * 4, p(buf), Cout, B, 1, 1, Cin, Cout, 1, 1, 1, 0, 0, 1, 1, 0, ops._stream())
    assert _lib.lib().mydet_conv2d_igemm_f32(p(x), Cin, p(wd), None, None, None, 0, *tail) == E_UNSUPP
    assert _lib.lib().mydet_conv2d_igemm_b3_f32(p(x), Cin, p(ops.split_bf16(wd)), None, None, None, 0, *tail) == E_UNSUPP
    torch.cuda.synchronize()
    assert _untouched(buf)


def test_guard_squeeze_forms_batch_65535(dev):
    """The squeeze forms launch an (S, B) grid: a 4 x 4, C = 16 map with squeeze=True is right at B = 65535 and MYDET_E_BADARG at
    65536 (the depthwise entry and the standalone squeeze); without the squeeze B = 70000 is right."""
    from mydetection_amd import _lib, ops
    C, k, s, pad = 16, 3, 1, (1, 1, 1, 1)
    g = _gen(dev, 81)
    w, wk, scale, shift = _dw_operands(dev, g, C, k)
    ref = _dw_ref(w, scale, shift, k, s, pad, C)

    def call(x):
        y, partial = ops.dwconv(x, wk, scale, shift, k, s, pad, ops.ACT_SWISH, squeeze=True)
        return y, partial[:, :-1]

    run_large(dev, 'dwconv squeeze B=65535', call, dict(x=randn_nhwc(g, 65535, C, 4, 4)), [abs_tol(2e-5), close_tol(1e-5, 1e-4)],
              lambda x: (ref(x), ref(x).sum(dim=(2, 3))), span='dwconv', exact=True, reduce=[None, lambda p: p.sum(dim=1)], crossing=False)
    x = randn_nhwc(g, 65536, C, 4, 4)
    with pytest.raises(_lib.MydetError, match='mydet_dwconv_f32 failed: bad argument'):
        ops.dwconv(x, wk, scale, shift, k, s, pad, ops.ACT_SWISH, squeeze=True)
    with pytest.raises(_lib.MydetError, match='mydet_channel_sums_f32 failed: bad argument'):
        ops.channel_sums(x)
    run_large(dev, 'dwconv B=70000', lambda x: ops.dwconv(x, wk, scale, shift, k, s, pad, ops.ACT_SWISH), dict(x=randn_nhwc(g, 70000, C, 4, 4)),
              [abs_tol(2e-5)], ref, span='dwconv', exact=True, crossing=False)
