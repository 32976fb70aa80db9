"""GPU tests of the box decode (csrc/decode.hip, called through ops.decode / ops.decode_levels as the product does) at
its edges, for every mode:

  * boxes and scores against the reference's float32 formulas (oracle/decoders.py) or the float64 RAPiD restatement
    (tests/test_rapid_host.py); clamped coordinates equal their bound exactly;
  * class ids on EVERY candidate, near-ties included, against the reference's rule -- torch.max over the float32
    sigmoids -- applied to the kernels' logistic 1 / (1 + exp(-x)) (common.h) on the device (where all of them
    underflow to 0, the largest logit, i.e. the float64 class); a float64 band guard keeps that oracle honest without
    trusting the device;
  * a geometry sweep through the plans of the host rule (mydet_decode_levels_f32: tile size PIX, lanes per candidate
    tpc, separate box staging registers, grid-stride loop with its register prefetch), and a tie sweep that puts an
    earlier and a later class a few float32 steps apart at every magnitude of the logistic;
  * the multi-level launch against per-level launches, bit for bit.
"""
import importlib.util
import os
import zlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

YOLO, RETINA, FCOS, RAPID = 0, 1, 2, 3          # ops.DECODE_* (asserted below)
PAD = 30.0                # channels the kernel must never read (anchor and row padding): a logit that would win if read
FLT_MIN = float(np.finfo(np.float32).tiny)
# A float32 logistic 1 / (1 + expf(-x)) is within 2 ulps of the float64 one (libm expf plus the two roundings), so two
# classes that share one float32 value lie within 4 ulps of each other in float64.
BAND_ULPS = 4

_spec = importlib.util.spec_from_file_location('rapid_host', os.path.join(os.path.dirname(__file__), 'test_rapid_host.py'))
_host = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_host)
rapid_f64 = _host.rapid_f64


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    from mydetection_amd import _lib, ops
    _lib.lib()
    assert (ops.DECODE_YOLO, ops.DECODE_RETINA, ops.DECODE_FCOS, ops.DECODE_RAPID) == (YOLO, RETINA, FCOS, RAPID)
    return torch.device('cuda:0')


# ------------------------------------------------------------------------------------------------------------ layouts
def _bw(mode):
    return 5 if mode == RAPID else 4


def _shared(mode, A, C, c0=0, apad=0, rpad=0):
    """One pixel-major tensor for box, objectness and classes: anchor a's block starts at a * astride + c0 and holds
    the box (4 or 5), the objectness (not RetinaNet) and the C class logits; apad / rpad floats of padding after
    each anchor block / at the end of the row (ld is a multiple of 4)."""
    bw = _bw(mode)
    conf = 0 if mode == RETINA else 1
    per = bw + conf + C + apad
    ld = (A * per + c0 + 3) // 4 * 4 + rpad
    return dict(same=True, box_astride=per, box_c0=c0, cls_astride=per, cls_c0=c0 + bw + conf,
                conf_c0=c0 + bw if conf else 0, ldbox=ld, ldcls=ld)


def _split(box_astride, box_c0, cls_astride, cls_c0, conf_c0, ldbox, ldcls):
    return dict(same=False, box_astride=box_astride, box_c0=box_c0, cls_astride=cls_astride, cls_c0=cls_c0,
                conf_c0=conf_c0, ldbox=ldbox, ldcls=ldcls)


def _plan(mode, A, C, B, sizes, L):
    """The host rule of mydet_decode_levels_f32 (decode.hip), restated: PIX pixels per tile, tpc lanes per candidate,
    float4 registers per thread for separate box rows (0: box rows come with the class rows), tiles of the largest
    level and the workgroups resident per level (more tiles than that: the grid-stride loop and its prefetch run).
    Each case states the path it takes; this keeps the statement true."""
    cls_need = (A - 1) * L['cls_astride'] + L['cls_c0'] + C
    if mode != RETINA:
        cls_need = max(cls_need, (A - 1) * L['cls_astride'] + L['conf_c0'] + 1)
    box_need = (A - 1) * L['box_astride'] + L['box_c0'] + _bw(mode)
    if L['same']:
        cls_need = max(cls_need, box_need)
    cls_span, box_span = (cls_need + 3) & ~3, (box_need + 3) & ~3
    row = (cls_span + (0 if L['same'] else box_span)) | 1
    qc, qb = cls_span // 4, box_span // 4

    def fits(pix):
        return pix * row * 4 <= 60 * 1024 and pix * qc <= 12 * 256 and (L['same'] or pix * qb <= 2 * 256)
    pix = 32
    while pix > 1 and not fits(pix):
        pix //= 2
    assert fits(pix)
    while pix * A < 256 and fits(pix * 2):
        pix *= 2
    tpc = 1 if C < 16 else (4 if pix * A <= 64 else (2 if pix * A <= 128 else 1))
    lds = (pix * row + 4) * 4
    per_cu = min(3, max(1, 160 * 1024 // (lds + 512)))
    return dict(pix=pix, tpc=tpc, nvb=0 if L['same'] else -(-pix * qb // 256),
                tiles=max(-(-B * h * w // pix) for h, w in sizes), resident=256 * per_cu)


def _pack(mode, t, conf, cls, L):
    """Logical logits t [B,A,H,W,bw], conf [B,A,H,W], cls [B,A,H,W,C] -> pixel-major numpy rows (box, cls); every
    channel no logit lands in holds PAD."""
    B, A, H, W = t.shape[:4]
    C, bw = cls.shape[-1], t.shape[-1]
    xc = np.full((B, H, W, L['ldcls']), PAD, np.float32)
    xb = xc if L['same'] else np.full((B, H, W, L['ldbox']), PAD, np.float32)
    a = np.arange(A)[:, None]
    bidx = a * L['box_astride'] + L['box_c0'] + np.arange(bw)
    cidx = a * L['cls_astride'] + L['cls_c0'] + np.arange(C)
    used_b, used_c = [bidx.ravel()], [cidx.ravel()]
    xb[..., bidx] = t.transpose(0, 2, 3, 1, 4)
    xc[..., cidx] = cls.transpose(0, 2, 3, 1, 4)
    if mode != RETINA:
        fidx = np.arange(A) * L['cls_astride'] + L['conf_c0']
        used_c.append(fidx)
        xc[..., fidx] = conf.transpose(0, 2, 3, 1)
    if L['same']:
        used_c += used_b
        used_b = used_c
    for used, ld in ((used_c, L['ldcls']), (used_b, L['ldbox'])):
        u = np.concatenate(used)
        assert len(np.unique(u)) == len(u) and u.max() < ld, 'overlapping or out-of-row channels in the case layout'
    return xb, xc


# ------------------------------------------------------------------------------------------------------------- inputs
# Tie sweep: ranges of the earlier class's logit x_j (weights), from where the float32 logistic keeps neighbouring
# logits apart (below -2) over where it merges most of them (-2 .. 17.4: the hole the old rule left) to saturation
# (>= 17.4: exactly 1) and the small / denormal logistics; dense in (-2, 5).
TIE_RANGES = [((-3.0, -1.0), 2.0), ((-2.0, 5.0), 8.0), ((-1.0, 5.0), 2.0), ((5.0, 15.0), 1.5), ((15.0, 17.5), 1.0),
              ((18.0, 40.0), 1.0), ((-88.7, -80.0), 1.0)]
UNDER, EQUAL = len(TIE_RANGES), len(TIE_RANGES) + 1     # all logistics 0 (x_j <= -89) / a row of equal logits


def _nextafter_n(x, n):
    for i in range(int(n.max(initial=0))):
        x = np.where(n > i, np.nextafter(x, np.float32(np.inf)), x)
    return x


def _inject_ties(cls, rng, frac):
    """At a fraction of the candidates: an earlier class j and a later class k with x_k = nextafter^n(x_j), n in
    {0, 1, 2, 3, 8} (0: an exact tie; j and k anywhere, so also in different lane shares), or x_k = x_j + a log-spaced
    gap up to 1e-3; every other class 20 .. 30 below.  Also pairs whose logistics underflow to 0 (x_j <= -89: the
    larger logit must win) and rows of one repeated logit.  Returns the mask of the underflow rows."""
    C = cls.shape[-1]
    x = cls.reshape(-1, C)
    rows = np.flatnonzero(rng.random(x.shape[0]) < frac)
    w = np.array([wt for _, wt in TIE_RANGES] + [0.5, 0.5])
    kind = rng.choice(len(w), size=rows.size, p=w / w.sum())
    lo = np.array([r[0] for r, _ in TIE_RANGES] + [-120.0, -2.0])[kind]
    hi = np.array([r[1] for r, _ in TIE_RANGES] + [-89.0, 5.0])[kind]
    xj = rng.uniform(lo, hi).astype(np.float32)
    x[rows] = (xj[:, None] - 20.0 - 10.0 * rng.random((rows.size, C))).astype(np.float32)
    if C > 1:
        j = rng.integers(0, C - 1, rows.size)
        k = j + 1 + (rng.random(rows.size) * (C - 1 - j)).astype(np.int64)
        xk = _nextafter_n(xj, rng.choice([0, 1, 1, 2, 3, 8], rows.size))
        gap = rng.random(rows.size) < 0.35
        xg = (xj.astype(np.float64) + 10.0 ** rng.uniform(-7.0, -3.0, rows.size)).astype(np.float32)
        xk = np.where(gap, np.maximum(xg, np.nextafter(xj, np.float32(np.inf))), xk)
        x[rows, j] = xj
        x[rows, k] = xk
    else:
        x[rows, 0] = xj
    under = kind == UNDER
    eq = kind == EQUAL
    x[rows[eq]] = xj[eq, None]
    mask = np.zeros(x.shape[0], bool)
    mask[rows[under]] = True
    return mask


def _inputs(mode, B, A, H, W, C, seed, ties, clamps):
    rng = np.random.default_rng(seed)
    t = (rng.standard_normal((B, A, H, W, _bw(mode))) * 1.5).astype(np.float32)
    if mode == RAPID:
        t[..., 4] = rng.uniform(-17.0, 17.0, (B, A, H, W))
    conf = (rng.standard_normal((B, A, H, W)) * 2.0).astype(np.float32)
    cls = (rng.standard_normal((B, A, H, W, C)) * 3.0 - 2.0).astype(np.float32)
    under = _inject_ties(cls, rng, ties)
    clamp = np.zeros((B, A, H, W), bool)
    if clamps:          # exp overflows to +inf / underflows to 0 and centres far out: every clamp of the mode is reached
        clamp = rng.random((B, A, H, W)) < 0.1
        n = int(clamp.sum())
        if mode == RETINA:
            t[clamp, 0:2] = rng.choice([-1e6, 1e6], (n, 2))
            t[clamp, 2:4] = rng.choice([-100.0, 100.0], (n, 2))
        else:   # FCOS: all four distances overflow -> the box is the whole image
            t[clamp] = 100.0
    return t, conf, cls, under.reshape(B, -1), clamp.reshape(B, -1)


def _anchors(A, seed):
    rng = np.random.default_rng(seed + 1)
    return (rng.uniform(8.0, 200.0, (A, 2))).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------ oracles
def _device_classes(cls, dev):
    """torch.max over 1 / (1 + exp(-x)) in float32 on the device: (max value, first index) per candidate.  Where every
    value is 0 (all logits below -88.7, where exp(-x) overflows) the first largest LOGIT: the exact logistics there are
    distinct float32 denormals, and the float64 class (what the model tests gate on) is that one."""
    B, C = cls.shape[0], cls.shape[-1]
    x = torch.from_numpy(np.ascontiguousarray(cls.reshape(B, -1, C))).to(dev)
    v, i = torch.max(1.0 / (1.0 + torch.exp(-x)), -1)
    i = torch.where(v == 0.0, torch.max(x, -1).indices, i)
    return v.cpu(), i.cpu().numpy()


def _check_band(cls, ci, ref_idx):
    """Device-independent guard: the chosen class's float64 logistic is within BAND_ULPS float32 ulps of the largest,
    and where that band holds one class it is the CPU reference's.  Rows whose largest logistic is below the float32
    normal range are left to the device oracle (there 1 / (1 + expf(-x)) drops to 0 past -88.7 while float64 does not)."""
    B, C = cls.shape[0], cls.shape[-1]
    p = 1.0 / (1.0 + np.exp(-cls.reshape(B, -1, C).astype(np.float64)))
    pm = p.max(-1)
    band = p >= (pm - BAND_ULPS * np.spacing(pm.astype(np.float32)).astype(np.float64))[..., None]
    ok = pm >= FLT_MIN
    chosen = np.take_along_axis(band, ci[..., None], -1)[..., 0]
    assert chosen[ok].all(), f'{int((~chosen & ok).sum())} class ids outside the float64 band'
    single = ok & (band.sum(-1) == 1)
    np.testing.assert_array_equal(ci[single], ref_idx[single])
    return int(single.sum()), int((ok & ~single).sum())


def _reference(mode, t, conf, cls, anchors, stride, img_hw):
    from oracle import decoders
    tt, cf, cl = (torch.from_numpy(a) for a in (t, conf, cls))
    if mode == YOLO:
        bb, idx, sc = decoders.yolo_decode_raw({'bbox': tt, 'conf': cf[..., None], 'class': cl}, stride, torch.from_numpy(anchors))
    elif mode == RETINA:
        bb, idx, sc = decoders.retina_decode({'bbox': tt, 'class': cl}, img_hw, stride, torch.from_numpy(anchors))
    elif mode == FCOS:
        bb, idx, sc = decoders.fcos_decode({'bbox': tt[:, 0], 'conf': cf[:, 0, ..., None], 'class': cl[:, 0]}, img_hw, stride)
    else:
        return rapid_f64(t, conf[..., None], cls, anchors, stride)
    return bb.double().numpy(), idx.numpy(), sc.double().numpy()


def _launch(mode, xb, xc, L, anchors, A, C, B, H, W, stride, img_hw, dev):
    from mydetection_amd import ops
    n = A * H * W
    out = (torch.full((B, n, _bw(mode)), np.nan, device=dev), torch.full((B, n), -1, dtype=torch.int64, device=dev),
           torch.full((B, n), np.nan, device=dev))
    db = torch.from_numpy(xb).to(dev)
    dc = db if L['same'] else torch.from_numpy(xc).to(dev)
    ops.decode(mode, db, L['ldbox'], L['box_astride'], L['box_c0'], dc, L['ldcls'], L['cls_astride'], L['cls_c0'],
               L['conf_c0'], anchors, A, C, B, H, W, stride, img_hw, *out, 0)
    return out


def _check_case(dev, mode, A, C, B, H, W, stride, L, ties, seed, clamps=False):
    t, conf, cls, under, clamp = _inputs(mode, B, A, H, W, C, seed, ties, clamps)
    anchors = None if mode == FCOS else _anchors(A, seed)
    img_hw = (H * stride, W * stride)           # the reference's anchor grid spans exactly W x H cells
    xb, xc = _pack(mode, t, conf, cls, L)
    bb, ci, sc = (o.cpu() for o in _launch(mode, xb, xc, L, anchors, A, C, B, H, W, stride, img_hw, dev))
    ci = ci.numpy()
    rb, ri, rs = _reference(mode, t, conf, cls, anchors, stride, img_hw)

    # class ids: exact on every candidate against the device oracle
    vmax, di = _device_classes(cls, dev)
    if mode == RETINA:          # precondition: the kernel's logistic IS the oracle's (score = max sigmoid, bit for bit)
        assert torch.equal(sc, vmax), 'kernel logistic differs from 1 / (1 + exp(-x)) on the device'
    bad = np.flatnonzero(ci.ravel() != di.ravel())
    assert bad.size == 0, (f'{bad.size} of {ci.size} class ids differ from torch.max over the float32 sigmoids; first '
                           f'at {bad[:4].tolist()}: kernel {ci.ravel()[bad[:4]].tolist()}, oracle {di.ravel()[bad[:4]].tolist()}')
    np.testing.assert_array_equal(ci[under], cls.reshape(B, -1, C).argmax(-1)[under], 'all logistics 0: the larger logit wins')
    _check_band(cls, ci, np.asarray(ri))

    # boxes and scores against the reference's formulas, in float64
    bb, sc = bb.double().numpy(), sc.double().numpy()
    if mode == RAPID:
        np.testing.assert_allclose(bb[..., :4], rb[..., :4], rtol=2e-6, atol=1e-5)
        np.testing.assert_allclose(bb[..., 4], rb[..., 4], rtol=0, atol=1e-4)
    elif mode == FCOS:          # x1, x2 round at the image's magnitude (expf may differ by an ulp between the host and
        # the device): the centre and width built from them carry two ulps of max(img_h, img_w) absolute
        np.testing.assert_allclose(bb, rb, rtol=2e-6, atol=max(1e-5, 2 * float(np.spacing(np.float32(max(img_hw))))))
    else:
        np.testing.assert_allclose(bb, rb, rtol=2e-6, atol=1e-6)
    np.testing.assert_allclose(sc, rs, rtol=2e-6, atol=1e-9)
    if mode == RETINA:          # clamped coordinates are their bound, exactly: [1, max(img_h, img_w)]
        hi = float(max(img_hw))
        at = (rb == 1.0) | (rb == hi)
        assert (not clamps) or (at.sum() > 0 and (rb == hi).any() and (rb == 1.0).any())
        np.testing.assert_array_equal(bb[at], rb[at])
        assert bb.min() >= 1.0 and bb.max() <= hi
    if mode == FCOS and clamps:  # both sides clamped to [0, img_w] / [0, img_h]: the whole image, exactly
        ih, iw = img_hw
        assert clamp.any()
        np.testing.assert_array_equal(bb[clamp], np.broadcast_to([iw / 2.0, ih / 2.0, float(iw), float(ih)], bb[clamp].shape))
    return t, cls


# ------------------------------------------------------------------------------------------------- the geometry sweep
# (id, mode, A, C, B, H, W, stride, layout, tie fraction, clamps, expected plan).  H * W is never a multiple of PIX with
# B > 1 (tiles straddle two images) and H != W (non-square images) except where a case says otherwise.
def _fcos_split(conf_c0, cls_c0, box_c0, ldbox, ldcls):
    return _split(4, box_c0, 0, cls_c0, conf_c0, ldbox, ldcls)


CASES = [
    # YOLO, one shared tensor, 85 channels per anchor: PIX 32, 96 candidates a tile -> tpc 2
    ('yolo_a3_c80', YOLO, 3, 80, 2, 13, 11, 32, _shared(YOLO, 3, 80, rpad=4), 0.5, False, dict(pix=32, tpc=2)),
    # YOLO, 128x128 level, B 2: 1024 tiles of 32 pixels > 768 resident workgroups -> grid-stride loop + prefetch
    ('yolo_grid_stride', YOLO, 3, 80, 2, 128, 128, 8, _shared(YOLO, 3, 80), 0.1, False, dict(pix=32, tpc=2, stride_loop=True)),
    # C 90 with the block at channel 3, 2 padding floats per anchor, padded row: PIX 32, tpc 2
    ('yolo_a3_c90_offsets', YOLO, 3, 90, 3, 7, 10, 16, _shared(YOLO, 3, 90, c0=3, apad=2, rpad=8), 0.6, False, dict(pix=32, tpc=2)),
    # C below 16: tpc 1 whatever the tile
    ('yolo_a3_c1', YOLO, 3, 1, 2, 9, 5, 32, _shared(YOLO, 3, 1, c0=1, rpad=4), 0.6, False, dict(tpc=1)),
    ('yolo_a3_c3', YOLO, 3, 3, 2, 9, 5, 32, _shared(YOLO, 3, 3, apad=1), 0.6, False, dict(tpc=1)),
    # RetinaNet, separate box [36] / class [720] rows: PIX 16, 144 candidates -> tpc 1, one box staging register
    ('retina_a9_c80', RETINA, 9, 80, 2, 10, 7, 16, _split(4, 0, 80, 0, 0, 36, 720), 0.5, True,
     dict(pix=16, tpc=1, nvb=1)),
    # RetinaNet 80x80, B 2: 800 tiles > 768 -> grid-stride loop + prefetch
    ('retina_grid_stride', RETINA, 9, 80, 2, 80, 80, 8, _split(4, 0, 80, 0, 0, 36, 720), 0.1, True,
     dict(pix=16, tpc=1, stride_loop=True)),
    # C 90, box rows 16 floats per anchor from channel 4, classes from channel 2 with 2 padding floats per anchor:
    # PIX 8, 72 candidates -> tpc 2; 272 box float4 a tile -> two box staging registers
    ('retina_a9_c90_offsets', RETINA, 9, 90, 2, 6, 11, 32, _split(16, 4, 92, 2, 0, 140, 832), 0.6, True,
     dict(pix=8, tpc=2, nvb=2)),
    # the largest accepted geometry: A 16, C 128 -> PIX 4, 64 candidates a tile -> tpc 4 (shares of 32 classes)
    ('retina_a16_c128', RETINA, 16, 128, 2, 9, 7, 16, _split(4, 0, 128, 0, 0, 68, 2052), 0.6, True,
     dict(pix=4, tpc=4, nvb=1)),
    # C below 16 (15 and 3): tpc 1
    ('retina_a9_c15', RETINA, 9, 15, 2, 7, 5, 64, _split(4, 0, 15, 1, 0, 40, 140), 0.6, True, dict(tpc=1)),
    ('retina_a9_c3', RETINA, 9, 3, 3, 5, 4, 128, _split(4, 0, 3, 0, 0, 36, 28), 0.6, True, dict(tpc=1)),
    # FCOS, conf at channel 0, classes 1..80 (the head's layout): PIX 128 -> tpc 2, one box staging register
    ('fcos_c80', FCOS, 1, 80, 2, 20, 13, 8, _fcos_split(0, 1, 0, 4, 84), 0.5, True, dict(pix=128, tpc=2, nvb=1)),
    # FCOS 160x160, B 4: 800 tiles of 128 pixels > 768 -> grid-stride loop + prefetch
    ('fcos_grid_stride', FCOS, 1, 80, 4, 160, 160, 8, _fcos_split(0, 1, 0, 4, 84), 0.1, True,
     dict(pix=128, tpc=2, stride_loop=True)),
    # FCOS C 128, conf at channel 0, box at channel 4 of 8: PIX 64 -> tpc 4
    ('fcos_c128', FCOS, 1, 128, 2, 11, 9, 16, _fcos_split(0, 1, 4, 8, 136), 0.6, True, dict(pix=64, tpc=4, nvb=1)),
    # FCOS C 16 (the smallest class count with lane shares), conf after the classes, box at channel 8 of 12:
    # PIX 128 -> tpc 2; 384 box float4 a tile -> two box staging registers
    ('fcos_c16', FCOS, 1, 16, 2, 15, 12, 8, _fcos_split(16, 0, 8, 12, 20), 0.6, True, dict(pix=128, tpc=2, nvb=2)),
    # FCOS C 17 (shares 5/5/5/2), conf at channel 120 makes the row long enough for PIX 64 -> tpc 4
    ('fcos_c17', FCOS, 1, 17, 2, 10, 9, 16, _fcos_split(120, 3, 0, 4, 128), 0.6, True, dict(pix=64, tpc=4)),
    # FCOS in one shared tensor (box 0..3, conf 4, classes 5..): PIX 128 -> tpc 2
    ('fcos_c90_shared', FCOS, 1, 90, 2, 19, 21, 8, _shared(FCOS, 1, 90, rpad=4), 0.5, True, dict(pix=128, tpc=2)),
    ('fcos_c15', FCOS, 1, 15, 2, 17, 9, 8, _fcos_split(15, 0, 0, 4, 16), 0.6, True, dict(tpc=1)),
    # RAPiD (5-float boxes), shared rows of 6 + C per anchor: C 80 -> PIX 32, tpc 2; C 20 -> PIX 128, tpc 1; C 3
    ('rapid_a3_c80', RAPID, 3, 80, 2, 9, 13, 16, _shared(RAPID, 3, 80, rpad=4), 0.6, False, dict(pix=32, tpc=2)),
    ('rapid_a3_c20', RAPID, 3, 20, 2, 11, 7, 16, _shared(RAPID, 3, 20, apad=2), 0.6, False, dict(pix=128, tpc=1)),
    ('rapid_a1_c3', RAPID, 1, 3, 3, 5, 9, 32, _shared(RAPID, 1, 3, c0=2), 0.6, False, dict(tpc=1)),
]


@pytest.mark.parametrize('case', CASES, ids=[c[0] for c in CASES])
def test_decode_geometry_sweep(dev, case):
    name, mode, A, C, B, H, W, stride, L, ties, clamps, want = case
    plan = _plan(mode, A, C, B, [(H, W)], L)
    for k in ('pix', 'tpc', 'nvb'):
        if k in want:
            assert plan[k] == want[k], (name, k, plan)
    assert plan['tiles'] > plan['resident'] if want.get('stride_loop') else plan['tiles'] <= plan['resident'], (name, plan)
    if not want.get('stride_loop'):
        assert B > 1 and (H * W) % plan['pix'] != 0 and H != W, 'tiles straddle images, the image is not square'
    _check_case(dev, mode, A, C, B, H, W, stride, L, ties, seed=zlib.crc32(name.encode()), clamps=clamps)


# ------------------------------------------------------------------------------------------------------ the tie sweep
# A tie at EVERY candidate, one case per mode and lane plan; the range of x_j cycles through TIE_RANGES (dense in
# (-2, 5), where neighbouring float32 logits share a logistic most often).
TIE_CASES = [
    ('yolo_tpc2', YOLO, 3, 80, 2, 24, 21, 8, _shared(YOLO, 3, 80)),
    ('retina_tpc1', RETINA, 9, 80, 2, 17, 12, 8, _split(4, 0, 80, 0, 0, 36, 720)),
    ('retina_tpc4', RETINA, 16, 128, 2, 9, 5, 32, _split(4, 0, 128, 0, 0, 64, 2048)),
    ('retina_tpc2', RETINA, 9, 90, 2, 11, 6, 16, _split(16, 4, 92, 2, 0, 140, 832)),
    ('fcos_tpc4', FCOS, 1, 128, 2, 30, 23, 8, _fcos_split(0, 1, 4, 8, 136)),
    ('fcos_tpc2', FCOS, 1, 80, 2, 40, 33, 8, _fcos_split(0, 1, 0, 4, 84)),
    ('fcos_c17_tpc4', FCOS, 1, 17, 2, 30, 21, 8, _fcos_split(120, 3, 0, 4, 128)),
    ('rapid_tpc2', RAPID, 3, 80, 2, 20, 17, 8, _shared(RAPID, 3, 80)),
    ('retina_c3_tpc1', RETINA, 9, 3, 2, 20, 15, 8, _split(4, 0, 3, 0, 0, 36, 28)),
]


@pytest.mark.parametrize('case', TIE_CASES, ids=[c[0] for c in TIE_CASES])
def test_decode_tie_sweep(dev, case):
    name, mode, A, C, B, H, W, stride, L = case
    _check_case(dev, mode, A, C, B, H, W, stride, L, ties=1.0, seed=zlib.crc32(b'ties ' + name.encode()))


# ----------------------------------------------------------------------------------------------- multi-level launches
LEVEL_CASES = [
    ('yolo', YOLO, 3, 80, [(20, 14), (10, 7), (5, 4)], [8, 16, 32], _shared(YOLO, 3, 80, rpad=4)),
    ('retina', RETINA, 9, 80, [(24, 18), (12, 9), (6, 5), (3, 3), (2, 2)], [8, 16, 32, 64, 128],
     _split(4, 0, 80, 0, 0, 36, 720)),
    ('fcos', FCOS, 1, 80, [(40, 30), (20, 15), (10, 8), (5, 4), (3, 2)], [8, 16, 32, 64, 128],
     _fcos_split(0, 1, 0, 4, 84)),
]


@pytest.mark.parametrize('case', LEVEL_CASES, ids=[c[0] for c in LEVEL_CASES])
def test_decode_levels_equal_per_level_launches(dev, case):
    from mydetection_amd import ops
    name, mode, A, C, sizes, strides, L = case
    B, img_hw = 2, (sizes[0][0] * strides[0], sizes[0][1] * strides[0])
    N = sum(A * h * w for h, w in sizes)
    one = (torch.full((B, N, 4), np.nan, device=dev), torch.full((B, N), -1, dtype=torch.int64, device=dev),
           torch.full((B, N), np.nan, device=dev))
    per_level = tuple(torch.full_like(o, -7) for o in one)
    levels, n_off = [], 0
    for i, ((h, w), st) in enumerate(zip(sizes, strides)):
        t, conf, cls, _, _ = _inputs(mode, B, A, h, w, C, seed=100 + i, ties=0.5, clamps=mode != YOLO)
        xb, xc = (torch.from_numpy(a).to(dev) for a in _pack(mode, t, conf, cls, L))
        xc = xb if L['same'] else xc
        anchors = None if mode == FCOS else _anchors(A, i)
        levels.append(dict(box=xb, ldbox=L['ldbox'], cls=xc, ldcls=L['ldcls'], anchors_wh=anchors, H=h, W=w, stride=st,
                           n_off=n_off))
        ops.decode(mode, xb, L['ldbox'], L['box_astride'], L['box_c0'], xc, L['ldcls'], L['cls_astride'], L['cls_c0'],
                   L['conf_c0'], anchors, A, C, B, h, w, st, img_hw, *per_level, n_off)
        n_off += A * h * w
    ops.decode_levels(mode, levels, L['box_astride'], L['box_c0'], L['cls_astride'], L['cls_c0'], L['conf_c0'], A, C, B,
                      img_hw, *one)
    for a, b in zip(one, per_level):
        assert torch.equal(a, b)
