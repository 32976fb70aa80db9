"""CPU tests of the lr_tb box head (EfficientDet + custom FCOS: configs d1_fcs2s / d1_fcs2s_mos): configuration and
state_dict against the reference's, constructor checks, the C ABI's argument checks, and a float64 restatement of the
layer pinned by fixtures made from the imported reference (tools/gen_golden_lr_tb.py)."""
import ctypes
import hashlib
import json

import numpy as np
import pytest
import torch
import torch.nn.functional as F


def lr_tb_f64(x, lr0, lr1, blr, tb0, tb1, btb):
    """_LR_TB_last (reference models/rpns.py:208-229) in float64: x [B,C,H,W] -> [B,4,H,W] (l, t, r, b)."""
    d = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float64)
    x = d(x)
    C = x.shape[1]
    dlr = F.conv2d(x, d(lr0), None, 1, 1, 1, C)
    dtb = F.conv2d(x, d(tb0), None, 1, 1, 1, C)
    lr = F.conv2d(dlr, d(lr1), d(blr), 1, (0, 1))          # the zero padding applies to the depthwise output
    tb = F.conv2d(dtb, d(tb1), d(btb), 1, (1, 0))
    return torch.stack([lr[:, 0], tb[:, 0], lr[:, 1], tb[:, 1]], dim=1)


def layer_weights(g):
    return (g['_lr_0_weight'], g['_lr_1_weight'], g['_lr_1_bias'], g['_tb_0_weight'], g['_tb_1_weight'], g['_tb_1_bias'])


@pytest.mark.parametrize('name', ['d1_fcs2s', 'd1_fcs2s_mos'])
def test_config_and_state_dict_match_the_reference(name, golden):
    from mydetection_amd import configs
    from mydetection_amd.models.general import name_to_model
    g = golden('d1_fcs2s_keys')
    ref_cfg = json.loads(str(g['cfg']))
    assert configs.get(name) == ref_cfg                   # the reference files' inference keys (_mos differs in train.* only)
    m, _ = name_to_model(name)
    sd = m.state_dict()
    assert list(sd) == [str(k) for k in g['keys']]
    assert [list(v.shape) for v in sd.values()] == json.loads(str(g['shapes']))
    assert sum(k.endswith(('._lr.0.weight', '._tb.1.bias')) for k in sd) == 10


def test_constructor_checks():
    from mydetection_amd import configs
    from mydetection_amd.models.rpns import EfDetHead, _LR_TB_last
    cfg = configs.get('d1_fcs2s')
    cfg['model.fpn.out_channels'] = [88] * 5
    head = EfDetHead(cfg)
    assert all(isinstance(net[-1], _LR_TB_last) for net in head.bbox_nets)
    bad = dict(cfg, **{'model.effrpn.num_anchor_per_level': 9})
    with pytest.raises(AssertionError):
        EfDetHead(bad)
    with pytest.raises(NotImplementedError):
        EfDetHead(dict(cfg, **{'model.effrpn.bbox_last': 'lr_tb_v2'}))


def test_abi_argument_checks():
    from mydetection_amd import _lib
    lib = _lib.lib()
    buf = (ctypes.c_float * 64)()                          # host memory: every call below must fail before touching it
    p = ctypes.cast(buf, ctypes.c_void_p).value
    p = (p + 15) // 16 * 16 if p % 16 else p

    def call(n=1, B=1, C=88, levels=None, **kw):
        lv = dict(x=p, ldx=C, w=p, y=p, ldy=4, H=5, W=5)
        lv.update(kw)
        arr = (_lib.LrTbLevel * 1)(_lib.LrTbLevel(**lv))
        ptr = None if levels == 'null' else ctypes.cast(arr, ctypes.c_void_p)
        return lib.mydet_lr_tb_levels_f32(n, ptr, B, C, None)
    bad = -1
    assert call(levels='null') == bad
    assert call(n=0) == bad and call(n=_lib.LR_TB_MAX_LEVELS + 1) == bad and call(B=0) == bad
    assert call(x=None) == bad and call(w=None) == bad and call(y=None) == bad
    assert call(C=86, ldx=88) == bad                       # C % 4 != 0
    assert call(C=_lib.LR_TB_MAX_C + 4, ldx=_lib.LR_TB_MAX_C + 4) == bad
    assert call(H=0) == bad and call(W=0) == bad and call(H=-3) == bad
    assert call(ldx=84) == bad                             # ldx < C
    assert call(ldy=2) == bad and call(ldy=6) == bad
    header = open(_lib.os.path.join(_lib._HERE, '..', 'include', 'mydet.h')).read()
    assert f'#define MYDET_LR_TB_MAX_LEVELS {_lib.LR_TB_MAX_LEVELS}' in header
    assert f'#define MYDET_LR_TB_MAX_C      {_lib.LR_TB_MAX_C}' in header


def test_float64_restatement_matches_the_reference_layer(golden):
    """Within 1e-6 x the output's RMS on every map (the fixture is the float32 reference: its round-off over the
    88-channel sums is ~7e-7 x RMS at 9x9)."""
    from mydetection_amd import synth
    g = golden('lr_tb_layer')
    B, C = int(g['B']), int(g['C'])
    for h, w in g['maps']:
        if f'x_{h}x{w}' in g:
            y = lr_tb_f64(g[f'x_{h}x{w}'], *layer_weights(g)).numpy()
            ref = g[f'y_{h}x{w}']
        else:                                              # the large map: input from its key, sampled output
            x = synth._normal(f'lr_tb_layer.x{h}x{w}', (B, C, h, w))
            y = lr_tb_f64(x, *layer_weights(g)).numpy().reshape(-1)
            np.testing.assert_allclose(np.sqrt((y ** 2).sum()), g[f'y_{h}x{w}_l2'], rtol=1e-6)
            y, ref = y[g[f'y_{h}x{w}_idx']], g[f'y_{h}x{w}_val']
        assert y.shape == ref.shape
        assert np.abs(y - ref).max() <= 1e-6 * np.sqrt((y ** 2).mean()), (h, w)


def test_restatement_in_the_oracle_forward_matches_the_reference_model(golden):
    """Backbone / BiFPN / towers of oracle.efficientdet, the box layer restated here, oracle.decoders.fcos_decode: the head
    bbox samples and all candidates of the 256^2 fixture within 1e-4."""
    from mydetection_amd import synth
    from mydetection_amd.models.general import name_to_model
    from oracle import efficientdet as oe
    from oracle.decoders import fcos_decode
    g = golden('d1_fcs2s_b1_256')
    m, _ = name_to_model('d1_fcs2s')
    sd = synth.make_state_dict(m.state_dict(), 'd1_fcs2s')
    x = synth.make_normalized_images(1, int(g['size']), seed=int(g['image_seed']))
    with torch.no_grad():
        feats = oe.bifpn(oe.backbone(x, sd, c6c7='conv'), sd)
        outs = []
        for lvl, f in enumerate(feats):
            towers = []
            for net in ('class_nets', 'bbox_nets'):
                t = f
                for r in range(3):
                    q = f'rpn.{net}.{lvl}.{r}'
                    t = oe._swish(oe._bn(oe.sepconv(t, sd, q + '.0'), sd, q + '.1'))
                towers.append(t)
            cls = oe.sepconv(towers[0], sd, f'rpn.class_nets.{lvl}.3')
            q = f'rpn.bbox_nets.{lvl}.3'
            box = lr_tb_f64(towers[1], sd[q + '._lr.0.weight'], sd[q + '._lr.1.weight'], sd[q + '._lr.1.bias'],
                            sd[q + '._tb.0.weight'], sd[q + '._tb.1.weight'], sd[q + '._tb.1.bias']).float()
            raw = {'bbox': box.permute(0, 2, 3, 1), 'conf': cls.permute(0, 2, 3, 1)[..., 0:1],
                   'class': cls.permute(0, 2, 3, 1)[..., 1:]}
            v = raw['bbox'].contiguous().numpy().reshape(-1)
            np.testing.assert_allclose(v[g[f'head_{lvl}_bbox_idx']], g[f'head_{lvl}_bbox_val'], rtol=1e-4, atol=1e-4)
            outs.append(fcos_decode(raw, tuple(x.shape[2:4]), oe.STRIDES[lvl]))
    boxes = torch.cat([o[0] for o in outs], 1)[0].numpy()
    scores = torch.cat([o[2] for o in outs], 1)[0].numpy()
    assert boxes.shape == g['bboxes_0'].shape == (1364, 4)
    np.testing.assert_allclose(scores, g['scores_0'], rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(boxes, g['bboxes_0'], rtol=1e-4, atol=1e-4)


# sha256 (first 16 hex digits) of make_state_dict of every configuration that existed before the lr_tb head, over
# (key, bytes) in state_dict order, both recipes for the EfficientNet-based ones: the new keys' recipe changed none of them
EXISTING_STATE_DICTS = {
    'yolov3_80': 'cea47b91e8ca12eb', 'efficientdet-d1': 'ec96b3877d4f68a7', 'd1_fcs2_atss': 'b97b479e560e67a7',
    'd1_fcs2': 'b97b479e560e67a7', 'd1_fcs': '435e8b713fac6332', 'd1_fcs2_p3': '4fcc0afb5f3a3e92',
    'd1_yv3': '1b2dbac5d06670cd', 'u5m_yv3': 'd1b16662b688d3e8', 'u5m_fcs2': '01fe5f8c093a213f'}


def test_synthetic_weights_of_existing_configs_unchanged():
    from mydetection_amd import synth
    from mydetection_amd.models.general import name_to_model
    for name, want in EXISTING_STATE_DICTS.items():
        m, cfg = name_to_model(name)
        h = hashlib.sha256()
        for recipe in ('conditioned', 'stiff') if 'efficientnet' in str(cfg.get('model.backbone.name')) else ('conditioned',):
            for k, v in synth.make_state_dict(m.state_dict(), name, recipe).items():
                h.update(k.encode())
                h.update(v.numpy().tobytes())
        assert h.hexdigest()[:16] == want, name


def test_lr_tb_synthetic_recipe():
    """The depthwise convs are plain conv weights, the (1,3) / (3,1) convs get the ltrb targets and the calibration the
    fixture ships (found through synth.load_calibration's fallback)."""
    from mydetection_amd import synth
    assert synth._efdet_last_kind('rpn.bbox_nets.2.3._lr.0.weight') is None
    assert synth._efdet_last_kind('rpn.bbox_nets.2.3._tb.0.weight') is None
    assert synth._efdet_last_kind('rpn.bbox_nets.2.3._tb.1.bias') == 'bbox'
    std, bias = synth._efdet_row_targets('bbox', 2)
    assert np.all(std == synth._EFDET_TARGETS['ltrb'][0]) and np.all(bias == synth._EFDET_TARGETS['ltrb'][1])
    calib = synth.load_calibration('d1_fcs2s')
    assert len(calib) == 304 and '__std__/rpn.bbox_nets.4.3._lr.1' in calib
    assert set(synth.load_calibration('d1_fcs2s_mos')) == set(calib)
