"""GPU: every shipped branch of the EfficientDet head and pyramid kernels against float64, at small shapes.

csrc/sepconv.hip (fused pyramid node, fused retina decode), the register-blocked depthwise kernels of csrc/mbconv.hip and the
skinny pointwise kernel of csrc/pointwise.hip pick an instantiation or a branch from the shape of a launch.  The models of the
suite (80 classes, 9 anchors, 88-channel square pyramids, depthwise layers of 16+ channels) reach only some of them.  Here
every one is run on purpose, and held to a float64 restatement of the same operation (tests/_refs.py).  Nothing is switched
through the environment: each case is a shape that the launch rules below send there.  Launch rules that depend on the chip
(the cuts of small grids) are restated in _decode_cut / _node_cut from multi_processor_count and asserted.

  case                               runs                                                          rule
  ---------------------------------  ------------------------------------------------------------  -------------------------
  A c1_nba6_levels  (90 cls, A 9)    sepconv_decode_kernel<22,6>, ragged 8x8 tiles, anchor cut     sepconv.hip:628, 667, 678
  A c1_unequal_cut  (90 cls, A 9)    <22,6>, slices of 2,2,2,2,1 anchors: a shorter last slice     sepconv.hip:442, 667-670
  A c2_81 / c2_96   (A 3)            <22,6>, an anchor's last block holds 1 / 16 classes           sepconv.hip:508
  A c3_65 / c3_72   (A 9, logits<-1) <22,5>, last block of 1 / 8 classes; only the mask keeps the  sepconv.hip:508, 676
                                     zero pad rows (logit 0) from beating every real class
  A c3_81_nba6      (A 9, logits<-1) <22,6>, the same with a last block of 1 class                 sepconv.hip:508, 678
  A c4_A1 / A4 / A12 (80 cls)        <22,5>; box node of 4 / 16 / 48 channels (shift clamp, an<A)  sepconv.hip:475, 538
  A c5_bn_scale                      <22,6>, P.scale != NULL in both node kinds                    sepconv.hip:478, 485
  A c6_uncut                         <22,6>, nsplit == 1 (tiles >= 2 x CUs)                        sepconv.hip:667
  A rejected 64 / 97                 MYDET_E_UNSUPP before any launch                              sepconv.hip:629
  B sweep, 2 inputs (0,1) (0,2)      sp_stage_halo<.., 0,1,-1> / <.., 0,2,-1>                      sepconv.hip:206-207
  B sweep, 3 inputs (0,0,2)          sp_stage_halo<.., 0,0,2>                                      sepconv.hip:208
  B sweep, the other 21 combinations sp_stage_halo_any (the branchy sp_read), n_in 2 and 3         sepconv.hip:209
  B weights all <= 0 / one positive  w = relu(w) / (sum + 1e-4) at sum == 0 / with one term        sepconv.hip:199-204
  B uncut, Cout 88 / 36              sepconv_kernel<22>, nsplit == 1, nb = 6 / 3 (odd; the last    sepconv.hip:607-612, 350
                                     block holds 4 channels)
  C 12x16                            dwconv_kernel / dwconv_sum_kernel <K,1,4,2> (dw_block2)       mbconv.hip:776-777, 781-783
  C 11x16                            dwconv_kernel / dwconv_sum_kernel <K,1,4>                     mbconv.hip:778, 784
  C 9x10                             dwconv_kernel / dwconv_sum_kernel <K,1,1>                     mbconv.hip:779, 785
    (C in {8, 12} < 16 keeps off the LDS-tiled kernel: mbconv.hip:849; K in {3, 5}; plain / squeeze sums / in-launch gate)
  D (tests/test_gpu_kernels.py::test_pointwise_skinny) pw_skinny_kernel<KC,NB,..,GATE>, KC = 4, 8, 10: pointwise.hip:210-222 (KC),
    180-190 (NB, slabs), 165-172 (gate).  64->24 gate <4,2,true>; 60->40 <4,3,false>, masked last chunk; 128->32 gate <8,2,true>;
    124->200 <8,5,false> x 3 slabs, masked last chunk; 160->40 gate <10,3,true>; 148->48 <10,3,false>, masked last chunk

Bounds (none is tuned to the kernels).  Conv outputs: the project's 2e-5 * max(1, max|ref|) (tests/test_gpu_kernels.py:
_conv_case).  Section A applies it to the logits, delta = 2e-5 * max(1, max|logit_ref|) per node, and carries it through
RetinaLayer's formulas: score 0.25 * delta + 2e-6 (the logistic's slope is at most 1/4; 2e-6 is the decode tests' score
tolerance), centres aw * delta + 2e-6 * |ref| + 1e-6, sizes |ref| * (delta + 4e-6) + 1e-6, a clamped value exact.  The class
index is compared wherever the two largest float64 logits are more than 2 * delta apart; the rest may be at most 0.5 % of a
case (the reference alone leaves out about 0.05 %: 200 000 rows of 65 .. 96 standard-normal logits on the CPU), and the cap is
asserted.  The fused decode must also give the bits of the two-launch device path (ops.sepconv_nodes writes the logits,
ops.decode reads them) and of its own second run.  ops.sepconv_nodes takes a Cout that is a multiple of 4, so where A * n_cls is
not, the two-launch class node carries one to three extra all-zero rows behind the last anchor, which the decode never reads."""
import functools

import pytest
import torch
import torch.nn.functional as F

from _refs import retina_decode_f64, se_gate_f64, sepconv_node_f64

pytestmark = pytest.mark.gpu

C = 88            # the instantiated channel count of sepconv.hip
GAP, TAIL = 7, 5  # candidates left unwritten between two levels' ranges (and in front of the first) and behind the last


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    from mydetection_amd import _lib
    _lib.lib()                                   # fail loudly if the HIP library is missing
    return torch.device('cuda:0')


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _tiles(hw):
    return ((hw[0] + 7) // 8) * ((hw[1] + 7) // 8)


# ----------------------------------------------------------------------------------------------- the launch rules, restated
def _decode_cut(cus, B, levels, A):
    """mydet_sepconv_decode_retina_f32's cut of the class nodes (sepconv.hip:661-670) for a launch of one class and one box node per
    level: the number of anchors per slice (A: uncut)."""
    base = sum(2 * B * _tiles(hw) for hw in levels)
    split = 1
    if base < 2 * cus:
        split = (3 * cus + base - 1) // base
    split = min(split, A)
    return (A + split - 1) // split


def _node_cut(cus, B, nodes_hw):
    """mydet_sepconv_nodes_f32 (sepconv.hip:598-612): True when the launch's nodes are cut along their output channels too."""
    return sum(B * _tiles(hw) for hw in nodes_hw) < cus


# ------------------------------------------------------------------------------------------------------- A. fused retina decode
def _anchors(A, stride):
    """RetinaLayer's anchor table: base 4 * stride, scales 2^(i/3) major, three ratios minor; the first A of it, as float32."""
    ratios = ((1.0, 1.0), (1.4, 0.7), (0.7, 1.4))
    return torch.tensor([[4.0 * stride * 2 ** ((a // 3) / 3) * ratios[a % 3][i] for i in (0, 1)] for a in range(A)], dtype=torch.float32)


def _uncut_batch(cus):
    return (cus + 63) // 64          # one 64 x 64 level: 64 tiles per node and image


def _unequal_level(cus):
    """A level of 40 x (8 r) pixels whose launch (B = 2) is cut into slices of 2 anchors when A = 9: 2,2,2,2,1."""
    return (max(1, round(0.45 * cus / 20)) * 8, 40)


RETINA_CASES = {
    'c1_nba6_levels': dict(seed=100, n_cls=90, A=9, levels=[(13, 9), (6, 5), (3, 3)]),
    'c1_unequal_cut': dict(seed=101, n_cls=90, A=9, levels='unequal', per=2),
    'c2_81': dict(seed=102, n_cls=81, A=3, levels=[(9, 7)]),
    'c2_96': dict(seed=103, n_cls=96, A=3, levels=[(9, 7)]),
    'c3_65': dict(seed=104, n_cls=65, A=9, levels=[(10, 10)], negative=True),
    'c3_72': dict(seed=105, n_cls=72, A=9, levels=[(10, 10)], negative=True),
    'c3_81_nba6': dict(seed=111, n_cls=81, A=9, levels=[(10, 10)], negative=True),
    'c4_A1': dict(seed=106, n_cls=80, A=1, levels=[(9, 7)]),
    'c4_A4': dict(seed=108, n_cls=80, A=4, levels=[(9, 7)]),
    'c4_A12': dict(seed=107, n_cls=80, A=12, levels=[(9, 7)]),
    'c5_bn_scale': dict(seed=109, n_cls=90, A=9, levels=[(11, 6)], bn=True),
    'c6_uncut': dict(seed=110, n_cls=90, A=3, levels=[(64, 64)], uncut=True),
}


@functools.lru_cache(maxsize=None)
def _retina_case(name, cus):
    """Inputs (CPU float32, seeded) and the float64 reference of a case, built once.  `cus` sizes the two chip-dependent cases."""
    c = dict(RETINA_CASES[name])
    g = torch.Generator().manual_seed(c['seed'])
    A, n_cls = c['A'], c['n_cls']
    B = _uncut_batch(cus) if c.get('uncut') else 2
    if c['levels'] == 'unequal':
        c['levels'] = [_unequal_level(cus)]
    strides = [8 << i for i in range(len(c['levels']))]
    c['img_hw'] = (c['levels'][0][0] * 8, c['levels'][0][1] * 8)
    n_off, lv = GAP, []
    for (H, W), stride in zip(c['levels'], strides):
        x = torch.randn(B, C, H, W, generator=g)
        L = dict(H=H, W=W, stride=stride, n_off=n_off, x=x, anchors=_anchors(A, stride))
        for kind, cout in (('cls', A * n_cls), ('box', A * 4)):
            w_dw = torch.randn(3, 3, C, generator=g) / 3.0
            w_pw = torch.randn(cout, C, generator=g) / C ** 0.5
            if kind == 'cls' and c.get('negative'):
                shift = -6.0 - torch.rand(cout, generator=g)
            else:
                shift = torch.randn(cout, generator=g) * 0.2
            scale = torch.rand(cout, generator=g) + 0.5 if c.get('bn') else None
            L[kind] = dict(w_dw=w_dw, w_pw=w_pw, shift=shift, scale=scale,
                           logits=sepconv_node_f64([x], [0], None, w_dw, w_pw, scale, shift, 0))
        L['ref'] = retina_decode_f64(L['cls']['logits'], L['box']['logits'], L['anchors'], stride, c['img_hw'])
        L['n'] = A * H * W
        n_off += L['n'] + GAP
        lv.append(L)
    c.update(B=B, lv=lv, N=n_off - GAP + TAIL, name=name)
    return c


def _sentinels(c, dev):
    B, N = c['B'], c['N']
    return (torch.full((B, N, 4), float('nan'), device=dev), torch.full((B, N), -1, dtype=torch.int64, device=dev),
            torch.full((B, N), float('nan'), device=dev))


def _nhwc(t, dev):
    return t.to(dev).contiguous(memory_format=torch.channels_last)


def _fused_nodes(c, dev):
    """The launch's node list, class nodes first (EfDetHead.decode_retina's order)."""
    from mydetection_amd import ops
    A, n_cls = c['A'], c['n_cls']
    cpad = (n_cls + 15) // 16 * 16
    nodes = []
    for kind in ('cls', 'box'):
        for L in c['lv']:
            p = L[kind]
            scale = p['scale']
            if kind == 'cls':
                w_pw, shift = ops.pack_pointwise_per_anchor(p['w_pw'], p['shift'], A, n_cls)
                if scale is not None:                      # the shift's per-anchor padded layout; pad entries 1.0
                    sp = torch.ones(A, cpad)
                    sp[:, :n_cls] = scale.view(A, n_cls)
                    scale = sp.view(-1)
            else:
                w_pw, shift = ops.pack_pointwise(p['w_pw']), p['shift']
            nodes.append(dict(inputs=[_nhwc(L['x'], dev)], w_dw=p['w_dw'].to(dev), w_pw=w_pw.contiguous().to(dev),
                              shift=shift.contiguous().to(dev), scale=scale.contiguous().to(dev) if scale is not None else None,
                              kind=0 if kind == 'cls' else 1, stride=L['stride'], anchors_wh=L['anchors'].numpy() if kind == 'box' else None,
                              n_off=L['n_off']))
    return nodes


def _run_fused(c, nodes, dev):
    from mydetection_amd import ops
    bbox, cidx, score = _sentinels(c, dev)
    ops.sepconv_decode_retina(nodes, c['A'], c['n_cls'], c['img_hw'], bbox, cidx, score)
    torch.cuda.synchronize()
    return bbox, cidx, score


def _run_two_launch(c, dev):
    """ops.sepconv_nodes writes the logits (anchor stride n_cls, unpadded), ops.decode in retina mode reads them."""
    from mydetection_amd import ops
    A, n_cls = c['A'], c['n_cls']
    nodes = []
    for kind in ('cls', 'box'):
        for L in c['lv']:
            p = L[kind]
            cout = p['w_pw'].shape[0]
            c4 = (cout + 3) // 4 * 4                       # sepconv_nodes: Cout % 4 == 0; the extra rows are zero and never decoded
            w = torch.zeros(c4, C)
            w[:cout] = p['w_pw']
            shift = torch.zeros(c4)
            shift[:cout] = p['shift']
            scale = None
            if p['scale'] is not None:
                scale = torch.ones(c4)
                scale[:cout] = p['scale']
            nodes.append(dict(inputs=[_nhwc(L['x'], dev)], modes=None, w_dw=p['w_dw'].to(dev), w_pw=ops.pack_pointwise(w).to(dev),
                              scale=scale.to(dev) if scale is not None else None, shift=shift.to(dev), cout=c4, act=ops.ACT_NONE))
    outs = ops.sepconv_nodes(nodes)
    n = len(c['lv'])
    bbox, cidx, score = _sentinels(c, dev)
    for L, cls, box in zip(c['lv'], outs[:n], outs[n:]):
        ops.decode(ops.DECODE_RETINA, box, ops.nhwc_ld(box), 4, 0, cls, ops.nhwc_ld(cls), n_cls, 0, 0, L['anchors'].numpy(), A, n_cls,
                   c['B'], L['H'], L['W'], L['stride'], c['img_hw'], bbox, cidx, score, L['n_off'])
    torch.cuda.synchronize()
    return bbox, cidx, score


def _same_bits(a, b):
    """Bit equality of two float tensors that may hold NaN sentinels."""
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def _held_retina(c, bbox, cidx, score):
    """Every check of a fused launch's outputs against the float64 reference.  Prints each figure before it asserts."""
    A, n_cls, name = c['A'], c['n_cls'], c['name']
    bbox, cidx, score = bbox.cpu(), cidx.cpu(), score.cpu()
    written = torch.zeros(c['N'], dtype=torch.bool)
    worst = dict(score=0.0, centre=0.0, size=0.0)
    left_out = total = 0
    hi = float(max(c['img_hw']))
    for li, L in enumerate(c['lv']):
        s = slice(L['n_off'], L['n_off'] + L['n'])
        written[s] = True
        ref = L['ref']
        bb, ci, sc = bbox[:, s].double(), cidx[:, s], score[:, s].double()
        assert bool(torch.isfinite(bb).all()) and bool(torch.isfinite(sc).all()), f'{name} level {li}: candidates not written'
        # class index: inside [0, n_cls) everywhere; the float64 argmax wherever the two largest logits are > 2 delta apart
        d_cls = 2e-5 * max(1.0, L['cls']['logits'].abs().max().item())
        assert int(ci.min()) >= 0 and int(ci.max()) < n_cls, f'{name} level {li}: class index outside [0, {n_cls}): {int(ci.min())} .. {int(ci.max())}'
        clear = ref['gap'] > 2 * d_cls
        left_out += int((~clear).sum())
        total += clear.numel()
        wrong = clear & (ci != ref['class_idx'])
        assert not bool(wrong.any()), f'{name} level {li}: {int(wrong.sum())} class indices differ from the float64 argmax; first {wrong.nonzero()[:4].tolist()}'
        e = ((sc - ref['score']).abs().max().item(), 0.25 * d_cls + 2e-6)
        worst['score'] = max(worst['score'], e[0] / e[1])
        print(f'effdet_branches A {name} level {li}: score err {e[0]:.3e} = {e[0] / e[1]:.3f} of the bound {e[1]:.3e}')
        assert e[0] <= e[1], f'{name} level {li}: score {e}'
        d_box = 2e-5 * max(1.0, L['box']['logits'].abs().max().item())
        err = (bb - ref['bbox']).abs()
        tol = torch.cat([ref['anchor'][..., :2] * d_box + 2e-6 * ref['bbox'][..., :2].abs() + 1e-6,
                         ref['bbox'][..., 2:].abs() * (d_box + 4e-6) + 1e-6], dim=-1)
        frac = err / tol
        worst['centre'] = max(worst['centre'], frac[..., :2].max().item())
        worst['size'] = max(worst['size'], frac[..., 2:].max().item())
        print(f'effdet_branches A {name} level {li}: centre err {err[..., :2].max().item():.3e} = {frac[..., :2].max().item():.3f} of its bound, '
              f'size err {err[..., 2:].max().item():.3e} = {frac[..., 2:].max().item():.3f} of its bound')
        assert bool((err <= tol).all()), f'{name} level {li}: box error {frac.max().item():.3f} of the bound at {(err > tol).nonzero()[:4].tolist()}'
        # a value the reference clamps by more than the bound is the clamp's own number
        raw_tol = torch.cat([ref['anchor'][..., :2] * d_box + 2e-6 * ref['raw'][..., :2].abs() + 1e-6,
                             ref['raw'][..., 2:].abs() * (d_box + 4e-6) + 1e-6], dim=-1)
        lo_c, hi_c = ref['raw'] < 1.0 - raw_tol, ref['raw'] > hi + raw_tol
        assert bool((bb[lo_c] == 1.0).all()) and bool((bb[hi_c] == hi).all()), f'{name} level {li}: a clamped value is not the clamp bound'
        if li == 0:
            assert bool(lo_c.any()) and bool(hi_c.any()), f'{name}: the case clamps nothing'
    share = left_out / total
    print(f'effdet_branches A {name}: {left_out} of {total} candidates ({100 * share:.3f} %) left out of the class comparison (cap 0.5 %); '
          f"worst score {worst['score']:.3f}, centre {worst['centre']:.3f}, size {worst['size']:.3f} of the bound")
    assert share <= 0.005, f'{name}: {100 * share:.3f} % of the candidates have their two largest logits within 2 delta'
    # outside the nodes' ranges (in front of the first, between two, behind the last) the sentinels stay
    out = ~written
    assert int(out.sum()) == GAP * len(c['lv']) + TAIL
    assert bool(torch.isnan(bbox[:, out]).all()) and bool(torch.isnan(score[:, out]).all()) and bool((cidx[:, out] == -1).all()), \
        f'{name}: candidates outside every node\'s range were written'


@pytest.mark.parametrize('name', list(RETINA_CASES))
def test_fused_retina_decode_vs_fp64(dev, name):
    """ops.sepconv_decode_retina stand-alone on hand-built nodes: against the float64 layer + RetinaLayer, the sentinels around the
    nodes' candidate ranges, the two-launch device path and a second run bit for bit."""
    cus = _cus()
    c = _retina_case(name, cus)
    A, n_cls = c['A'], c['n_cls']
    per = _decode_cut(cus, c['B'], c['levels'], A)
    if c.get('uncut'):               # the launch's tiles, summed over its nodes, are at least twice the CU count: no anchor cut
        assert sum(2 * c['B'] * _tiles(hw) for hw in c['levels']) >= 2 * cus and per == A, (cus, c['B'], c['levels'])
    else:
        assert per < A or A == 1, (cus, per)
        if 'per' in c:               # slices of `per` anchors that do not divide A: a shorter last slice
            assert per == c['per'] and A % per != 0, (cus, c['levels'], per)
    if c.get('negative'):            # every real logit is far below the 0 of a padded row
        assert all(L['cls']['logits'].max().item() < -1.0 for L in c['lv'])
    nodes = _fused_nodes(c, dev)
    bbox, cidx, score = _run_fused(c, nodes, dev)
    _held_retina(c, bbox, cidx, score)
    bbox2, cidx2, score2 = _run_fused(c, nodes, dev)
    assert _same_bits(bbox, bbox2) and torch.equal(cidx, cidx2) and _same_bits(score, score2), f'{name}: a second run differs'
    bbox3, cidx3, score3 = _run_two_launch(c, dev)
    assert _same_bits(score, score3), f'{name}: scores differ from the two-launch path'
    assert torch.equal(cidx, cidx3), f'{name}: class indices differ from the two-launch path'
    assert _same_bits(bbox, bbox3), f'{name}: boxes differ from the two-launch path'


@pytest.mark.parametrize('n_cls', [64, 97])
def test_fused_retina_decode_rejects_other_class_counts(dev, n_cls):
    """4 and 7 channel blocks per anchor are not instantiated: MYDET_E_UNSUPP, and nothing is written."""
    from mydetection_amd import _lib, ops
    g = torch.Generator().manual_seed(n_cls)
    A, B, H, W = 3, 2, 9, 7
    x = _nhwc(torch.randn(B, C, H, W, generator=g), dev)
    w_cls, sh_cls = ops.pack_pointwise_per_anchor(torch.randn(A * n_cls, C, generator=g) / C ** 0.5, torch.randn(A * n_cls, generator=g), A, n_cls)
    nodes = [dict(inputs=[x], w_dw=(torch.randn(3, 3, C, generator=g) / 3.0).to(dev), w_pw=w_cls.to(dev), shift=sh_cls.to(dev), scale=None,
                  kind=0, stride=8, anchors_wh=None, n_off=0),
             dict(inputs=[x], w_dw=(torch.randn(3, 3, C, generator=g) / 3.0).to(dev),
                  w_pw=ops.pack_pointwise(torch.randn(A * 4, C, generator=g) / C ** 0.5).to(dev), shift=torch.randn(A * 4, generator=g).to(dev),
                  scale=None, kind=1, stride=8, anchors_wh=_anchors(A, 8).numpy(), n_off=0)]
    c = dict(B=B, N=A * H * W + TAIL)
    bbox, cidx, score = _sentinels(c, dev)
    with pytest.raises(_lib.MydetError, match='unsupported configuration'):
        ops.sepconv_decode_retina(nodes, A, n_cls, (72, 56), bbox, cidx, score)
    torch.cuda.synchronize()
    assert bool(torch.isnan(bbox).all()) and bool(torch.isnan(score).all()) and bool((cidx == -1).all())


# ----------------------------------------------------------------------------------------------------- B. fused pyramid node
PAIRS = [(0, 0), (1, 0), (2, 0), (0, 1), (0, 2)]
TRIPLES = [(a, b, c_) for a in range(3) for b in range(3) for c_ in range(3) if 0 in (a, b, c_)]
assert len(TRIPLES) == 19


def _node(g, B, hw, modes, cout, act, bn, fuse_w=None):
    H, W = hw
    shapes = {0: (H, W), 1: (H // 2, W // 2), 2: (H * 2, W * 2)}
    n_in = len(modes)
    if fuse_w is None and n_in > 1:
        fuse_w = torch.randn(n_in, generator=g)
        fuse_w[0] = fuse_w[0].abs() + 0.2                  # at least one positive weight; the others are negative about half the time
    nd = dict(inputs=[torch.randn(B, C, *shapes[m], generator=g) for m in modes], modes=list(modes), fuse_w=fuse_w,
              w_dw=torch.randn(3, 3, C, generator=g) / 3.0, w_pw=torch.randn(cout, C, generator=g) / C ** 0.5,
              scale=torch.rand(cout, generator=g) + 0.5 if bn else None, shift=torch.randn(cout, generator=g) * 0.2, cout=cout, act=act)
    nd['ref'] = sepconv_node_f64(nd['inputs'], nd['modes'], nd['fuse_w'], nd['w_dw'], nd['w_pw'], nd['scale'], nd['shift'], act)
    return nd


@functools.lru_cache(maxsize=None)
def _sweep_nodes():
    """One node per input-mode combination, B = 2, Cout = 88, maps 10x6 and 8x8 in turn, swish / none and BN / bias in turn."""
    g = torch.Generator().manual_seed(31)
    return [_node(g, 2, ((10, 6), (8, 8))[i % 2], modes, 88, (2, 0)[(i // 2) % 2], i % 3 != 0) for i, modes in enumerate(PAIRS + TRIPLES)]


def _device_node(nd, dev):
    from mydetection_amd import ops
    return dict(inputs=[_nhwc(t, dev) for t in nd['inputs']], modes=nd['modes'],
                fuse_weights=nd['fuse_w'].to(dev) if nd['fuse_w'] is not None else None, w_dw=nd['w_dw'].to(dev),
                w_pw=ops.pack_pointwise(nd['w_pw']).to(dev), scale=nd['scale'].to(dev) if nd['scale'] is not None else None,
                shift=nd['shift'].to(dev), cout=nd['cout'], act=nd['act'])


def _held_nodes(grp, dev, what):
    """One launch of `grp`: against float64, the three launches it replaces, and a second run.  Returns the outputs."""
    from mydetection_amd import ops
    dn = [_device_node(nd, dev) for nd in grp]
    outs = ops.sepconv_nodes(dn)
    again = ops.sepconv_nodes(dn)
    torch.cuda.synchronize()
    for nd, d, y, y2 in zip(grp, dn, outs, again):
        ref = nd['ref']
        assert tuple(y.shape) == tuple(ref.shape)
        yc = y.cpu().double()
        assert bool(torch.isfinite(yc).all())
        tol = 2e-5 * max(1.0, ref.abs().max().item())
        err = (yc - ref).abs().max().item()
        print(f"effdet_branches B {what} modes {tuple(nd['modes'])} {ref.shape[2]}x{ref.shape[3]} cout {nd['cout']}: err {err:.3e} = "
              f'{err / tol:.3f} of the bound {tol:.3e}')
        assert err <= tol, (what, nd['modes'], err, tol)
        assert torch.equal(y, y2), (what, nd['modes'], 'a second run differs')
        x = ops.bifpn_fuse(d['inputs'], d['modes'], d['fuse_weights']) if len(d['inputs']) > 1 else d['inputs'][0]
        t = ops.dwconv(x, d['w_dw'], None, None, 3, 1, (1, 1, 1, 1), ops.ACT_NONE)
        old = ops.conv2d(t, nd['w_pw'].reshape(nd['cout'], 1, 1, C).to(dev), d['scale'], d['shift'], 1, 1, (0, 0, 0, 0), nd['act'])
        diff = (y - old).abs().max().item()
        assert diff <= 0.5 * tol, (what, nd['modes'], 'three-launch path', diff, 0.5 * tol)      # 1e-5 * max(1, max|ref|)
    return outs


@pytest.mark.parametrize('part', [0, 1, 2])
def test_sepconv_every_input_mode_combination(dev, part):
    """All 5 two-input and 19 three-input mode combinations, eight nodes to a launch (small grids: cut along the channels)."""
    nodes = _sweep_nodes()
    grp = nodes[part * 8:(part + 1) * 8]
    assert len(grp) == 8 and _node_cut(_cus(), 2, [nd['ref'].shape[2:] for nd in grp])
    if part == 2:
        assert {tuple(nd['modes']) for nd in nodes} == set(PAIRS + TRIPLES)
    _held_nodes(grp, dev, f'sweep {part}')


def test_sepconv_fusion_weight_edges(dev):
    """Fusion weights all <= 0: w = 0 / 1e-4 = 0, the pre-activation is exactly 0 and the node's output is its bias after BN, to
    the bit.  One positive weight among negative ones: w = (0, p / (p + 1e-4), 0)."""
    g = torch.Generator().manual_seed(32)
    grp = [_node(g, 2, (10, 6), (0, 1, 2), 88, 0, True, fuse_w=torch.tensor([-0.7, 0.0, -1.5])),
           _node(g, 2, (8, 8), (0, 2), 88, 0, False, fuse_w=torch.tensor([0.0, -0.2])),
           _node(g, 2, (8, 8), (1, 0, 0), 88, 2, True, fuse_w=torch.tensor([-0.3, 0.9, -1.0])),
           _node(g, 2, (10, 6), (0, 1), 88, 2, True, fuse_w=torch.tensor([-0.3, 0.9]))]
    outs = _held_nodes(grp, dev, 'fusion edges')
    for nd, y in zip(grp[:2], outs[:2]):
        assert torch.equal(y.cpu(), nd['shift'].view(1, -1, 1, 1).expand_as(y)), 'all weights <= 0: the output is not the bias'


@pytest.mark.parametrize('cout', [88, 36])
def test_sepconv_uncut_launch(dev, cout):
    """A launch with at least as many tiles as CUs: every workgroup walks all channel blocks of its tile (nsplit == 1), six of
    them, or three with a last block of four channels."""
    import os
    assert 'MYDET_SEPCONV_SPLIT' not in os.environ
    cus = _cus()
    B = _uncut_batch(cus)
    assert not _node_cut(cus, B, [(64, 64)]), (cus, B)
    g = torch.Generator().manual_seed(33 + cout)
    _held_nodes([_node(g, B, (64, 64), (0, 1), cout, 2, True)], dev, f'uncut B {B}')


# ------------------------------------------------------------------------------------- C. register-blocked depthwise kernels
@pytest.mark.parametrize('H,W', [(12, 16), (11, 16), (9, 10)])
@pytest.mark.parametrize('k', [3, 5])
@pytest.mark.parametrize('Cd', [8, 12])
def test_dwconv_register_blocked(dev, Cd, k, H, W):
    """Stride 1 under 16 channels: the three forms of launch_dw (two-row blocks, four-wide strips, single outputs), each plain,
    with the squeeze sums and with the in-launch gate -- the checks of test_dwconv and test_se_gate_inside_depthwise_launch."""
    from mydetection_amd import ops
    g = torch.Generator().manual_seed(Cd * 1000 + k * 100 + H)
    B, Cse, p = 2, 4, (k - 1) // 2
    x = torch.randn(B, Cd, H, W, generator=g)
    w = torch.randn(Cd, 1, k, k, generator=g) * 0.3
    scale, shift = torch.rand(Cd, generator=g) + 0.5, torch.randn(Cd, generator=g) * 0.1
    w1, b1 = torch.randn(Cse, Cd, generator=g) / Cd ** 0.5, torch.randn(Cse, generator=g) * 0.1
    w2t, b2 = torch.randn(Cse, Cd, generator=g) * 0.3, torch.randn(Cd, generator=g) * 0.1
    ref = F.conv2d(x.double(), w.double(), None, 1, p, 1, Cd) * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1)
    ref = ref * torch.sigmoid(ref)
    assert ref.shape[2:] == (H, W)
    args = (_nhwc(x, dev), w.permute(2, 3, 0, 1).reshape(k, k, Cd).contiguous().to(dev), scale.to(dev), shift.to(dev), k, 1, (p,) * 4,
            ops.ACT_SWISH)
    se = tuple(t.contiguous().to(dev) for t in (w1, b1, w2t, b2))
    y = ops.dwconv(*args)
    err = (y.cpu().double() - ref).abs().max().item()
    print(f'effdet_branches C C{Cd} k{k} {H}x{W}: err {err:.3e} = {err / 2e-5:.3f} of the bound 2e-5')
    assert err < 2e-5
    y2, partial = ops.dwconv(*args, squeeze=True)
    assert torch.equal(y2.contiguous(), y.contiguous()), 'the squeeze form writes another map'
    sums, ref_sums = partial[:, :-1].sum(dim=1).cpu().double(), ref.sum(dim=(2, 3))
    print(f'effdet_branches C C{Cd} k{k} {H}x{W}: slice-sum err {(sums - ref_sums).abs().max().item():.3e} (rtol 1e-5, atol 1e-4)')
    torch.testing.assert_close(sums, ref_sums, rtol=1e-5, atol=1e-4)
    y3, gate = ops.dwconv(*args, se=se)
    assert torch.equal(y3.contiguous(), y.contiguous()), 'the gate form writes another map'
    assert tuple(gate.shape) == (B, Cd)
    gerr = (gate.cpu().double() - se_gate_f64(ref, w1, b1, w2t, b2)).abs().max().item()
    print(f'effdet_branches C C{Cd} k{k} {H}x{W}: gate err {gerr:.3e} = {gerr / 3e-6:.3f} of the bound 3e-6')
    assert gerr < 3e-6
    for _ in range(2):
        y4, gate4 = ops.dwconv(*args, se=se)
        assert torch.equal(gate4, gate) and torch.equal(y4.contiguous(), y.contiguous())
