"""CPU tests of the Ultralytics (YOLOv5) decode layer and the ulo5m configuration: registry, configuration and state_dict
against the reference's (tools/gen_golden_uv5.py), the synthetic weights, the float32 restatement the decode kernel
implements pinned bit for bit by the reference layer's fixture, the argument checks of the new C entry point, and the
layer's refusals."""
import ctypes
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

_spec = importlib.util.spec_from_file_location('rapid_host_for_uv5', os.path.join(os.path.dirname(__file__), 'test_rapid_host.py'))
_rapid_host = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_rapid_host)


def _grid(H, W, dtype):
    gy, gx = np.meshgrid(np.arange(H, dtype=dtype), np.arange(W, dtype=dtype), indexing='ij')
    return gx, gy


def uv5_f32(t, conf, cls, anchors, stride):
    """DetectLayer's inference branch (reference models/detlayers/uv5.py:42-91) restated in float32, every operation rounded
    on its own in the order the decode kernel keeps: ((s*2 - 0.5) + g) * stride and ((s*2) * (s*2)) * anchor, with s, the
    objectness and the class probabilities torch's float32 sigmoid.  t [B,A,H,W,4], conf [B,A,H,W,1], cls [B,A,H,W,C] ->
    (bbox [B,N,4] f32, class_idx [B,N] i64, score [B,N] f32)."""
    B, A, H, W, _ = t.shape
    s = torch.sigmoid(torch.from_numpy(np.ascontiguousarray(t, np.float32))).numpy()
    two, half, st = np.float32(2), np.float32(0.5), np.float32(stride)
    gx, gy = _grid(H, W, np.float32)
    aw = np.asarray(anchors, np.float32)[:, 0].reshape(1, A, 1, 1)
    ah = np.asarray(anchors, np.float32)[:, 1].reshape(1, A, 1, 1)
    w2, h2 = s[..., 2] * two, s[..., 3] * two
    box = np.stack([((s[..., 0] * two - half) + gx) * st, ((s[..., 1] * two - half) + gy) * st, (w2 * w2) * aw, (h2 * h2) * ah], -1)
    assert box.dtype == np.float32
    cmax, idx = torch.sigmoid(torch.from_numpy(np.ascontiguousarray(cls, np.float32))).max(-1)
    score = torch.sigmoid(torch.from_numpy(np.ascontiguousarray(conf, np.float32)))[..., 0] * cmax
    return box.reshape(B, -1, 4), idx.numpy().reshape(B, -1), score.numpy().reshape(B, -1)


def uv5_f64(t, conf, cls, anchors, stride):
    """The same layer in float64: (bbox [B,N,4], class_idx [B,N], score [B,N], top-two class-probability gap [B,N])."""
    t, conf, cls = (np.asarray(a, np.float64) for a in (t, conf, cls))
    B, A, H, W, _ = t.shape
    sig = lambda v: 1.0 / (1.0 + np.exp(-v))
    gx, gy = _grid(H, W, np.float64)
    aw = np.asarray(anchors, np.float64)[:, 0].reshape(1, A, 1, 1)
    ah = np.asarray(anchors, np.float64)[:, 1].reshape(1, A, 1, 1)
    s = sig(t)
    box = np.stack([(s[..., 0] * 2 - 0.5 + gx) * stride, (s[..., 1] * 2 - 0.5 + gy) * stride, (s[..., 2] * 2) ** 2 * aw,
                    (s[..., 3] * 2) ** 2 * ah], -1)
    p = sig(cls)
    top = np.sort(p, -1)
    gap = top[..., -1] - top[..., -2] if p.shape[-1] > 1 else np.ones(p.shape[:-1])
    score = sig(conf[..., 0]) * p.max(-1)
    return box.reshape(B, -1, 4), p.argmax(-1).reshape(B, -1), score.reshape(B, -1), gap.reshape(B, -1)


def test_registry_config_and_state_dict_match_the_reference(golden):
    from mydetection_amd import configs
    from mydetection_amd.models import registry
    from mydetection_amd.models.detlayers.uv5 import DetectLayer
    from mydetection_amd.models.general import name_to_model, state_dict_template
    g = golden('uv5_keys')
    cfg = configs.get('ulo5m')
    assert 'ulo5m' in configs.NAMES
    assert cfg == json.loads(str(g['ulo5m_cfg']))            # the reference file's inference keys, exactly
    assert cfg['model.pred_layer'] == 'Ultralytics' and registry.get_det_layer(cfg) is DetectLayer
    tpl = state_dict_template('ulo5m')
    assert list(tpl) == [str(k) for k in g['ulo5m_keys']] and len(tpl) == 462
    assert [list(v.shape) for v in tpl.values()] == json.loads(str(g['ulo5m_shapes']))
    m, cfg = name_to_model('ulo5m')
    assert list(m.state_dict()) == list(tpl)
    assert all(type(d) is DetectLayer for d in m.det_layers) and len(m.det_layers) == 3
    assert m.bbox_param == 4 and m.bb_format == 'cxcywh' and m.batch_lanes_hint == 1
    assert cfg['model.fpn.out_strides'] == [8, 16, 32]


def test_detect_layer_constructor_and_refusals():
    from mydetection_amd import configs
    from mydetection_amd.models.detlayers.uv5 import DetectLayer
    cfg = configs.get('ulo5m')
    cfg['model.fpn.out_strides'] = [8, 16, 32]
    layer = DetectLayer(1, cfg)
    assert layer.num_anchors == 3 and layer.stride == 16 and layer.n_cls == 80
    assert layer.indices.tolist() == [3, 4, 5]
    np.testing.assert_array_equal(layer.anchors.numpy(), np.float32([[30, 61], [62, 45], [59, 119]]))
    assert layer.anch_00wh_all.shape == (9, 4) and not layer.anch_00wh_all[:, :2].any()
    np.testing.assert_array_equal(layer.anch_00wh_all[:, 2:].numpy(), np.float32(cfg['model.detect.anchors']))
    # the keys only the training branch reads are optional
    lean = {k: v for k, v in cfg.items() if k not in ('model.detect.sample_selection', 'model.detect.confidence_target',
                                                      'model.detect.loss_bbox', 'model.detect.negative_threshold')}
    assert DetectLayer(0, lean).stride == 8
    raw = {'bbox': torch.zeros(1, 3, 2, 2, 4), 'conf': torch.zeros(1, 3, 2, 2, 1), 'class': torch.zeros(1, 3, 2, 2, 80)}
    with pytest.raises(NotImplementedError):
        layer(raw, (32, 32), labels=[])
    rotated = DetectLayer(1, dict(cfg, **{'general.pred_bbox_format': 'cxcywhd'}))
    with pytest.raises(NotImplementedError):
        rotated(raw, (32, 32))
    assert rotated._describe(raw, (32, 32)) is None


# the RAPiD configurations, pinned like the eleven older ones of tests/test_rapid_host.py (same hash)
RAPID_STATE_DICTS = {'rapid': '33d2533b5f01771d', 'rapid_psl1': '33d2533b5f01771d', 'yv3_pl1_80': '1b71502f9fe9d5bd',
                     'u5m_rapid': 'c66ec138d051757c', 'd1_rapid': 'b6bc101be9c04dca'}


def test_synthetic_weights_equal_u5m_yv3_and_leave_every_config_pinned():
    from mydetection_amd import synth
    from mydetection_amd.models.general import state_dict_template
    a = synth.make_state_dict(state_dict_template('ulo5m'), 'ulo5m')
    b = synth.make_state_dict(state_dict_template('u5m_yv3'), 'u5m_yv3')
    assert list(a) == list(b)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert _rapid_host._state_dict_hash('ulo5m') == _rapid_host.EXISTING_STATE_DICTS['u5m_yv3']
    for name, want in {**_rapid_host.EXISTING_STATE_DICTS, **RAPID_STATE_DICTS}.items():
        assert _rapid_host._state_dict_hash(name) == want, name


def test_float32_restatement_equals_the_reference_layer_bit_for_bit(golden):
    """What csrc/decode.hip computes for this layer, operation by operation, on the reference layer's own fixture: boxes and
    scores bit for bit, class ids exactly; the float64 form agrees within float32 round-off; the fixture reaches the ends
    of the parameterisation (cx = -stride/2, w = 4 * anchor, w -> 0)."""
    g = golden('uv5_layer')
    ends = {'low': 0, 'wide': 0, 'thin': 0}
    for n_cls in (1, 80):
        for lvl, (h, w) in enumerate(g['maps']):
            key = f'c{n_cls}_{h}x{w}'
            t, conf, cls = g[f'{key}_bbox_in'], g[f'{key}_conf_in'], g[f'{key}_class_in']
            anchors, stride = g[f'{key}_anchors'], float(g['strides'][lvl])
            ref_box, ref_idx, ref_score = g[f'{key}_bbox'], g[f'{key}_class_idx'], g[f'{key}_score']
            assert t.shape == (2, 3, h, w, 4) and cls.shape[-1] == n_cls and ref_box.shape == (2, 3 * h * w, 4)
            assert np.abs(t).max() > 19.0
            box, idx, score = uv5_f32(t, conf, cls, anchors, stride)
            np.testing.assert_array_equal(box, ref_box)
            np.testing.assert_array_equal(score, ref_score)
            np.testing.assert_array_equal(idx, ref_idx)
            box64, idx64, score64, gap = uv5_f64(t, conf, cls, anchors, stride)
            np.testing.assert_allclose(ref_box, box64, rtol=1e-6, atol=1e-5)
            np.testing.assert_allclose(ref_score, score64, rtol=1e-6, atol=1e-9)
            safe = gap > 1e-6
            assert safe.mean() > 0.99
            np.testing.assert_array_equal(ref_idx[safe], idx64[safe])
            a4 = 4 * np.tile(np.repeat(anchors, h * w, 0), (2, 1)).reshape(2, -1, 2)
            assert (ref_box[..., 2:] <= a4).all() and (ref_box[..., :2] >= -stride / 2).all()
            ends['low'] += int((ref_box[..., :2] == -stride / 2).sum())
            ends['wide'] += int((ref_box[..., 2:] == a4).sum())
            ends['thin'] += int((ref_box[..., 2:] < 1e-6 * a4).sum())
    assert min(ends.values()) >= 1, ends                  # (cx = -stride/2 needs a cell of column 0 or row 0)


def test_abi_argument_checks_of_the_uv5_entry():
    """The new entry point rejects bad arguments before any launch (host pointers only: a call that got past the checks
    would fault), and the public mode argument did not grow."""
    from mydetection_amd import _lib
    lib = _lib.lib()
    buf = (ctypes.c_float * 256)()
    p = ctypes.cast(buf, ctypes.c_void_p).value
    p = (p + 15) // 16 * 16
    anch = (ctypes.c_float * 32)(*([10.0] * 32))
    anch_p = ctypes.cast(anch, ctypes.c_void_p).value

    def uv5(A=3, C=1, box=p, bbox=p, cidx=p, score=p, anchors=anch_p, ld=20, H=2, W=2, nlevels=1, levels=True, N=None):
        lv = _lib.DecodeLevel(box, ld, box, ld, anchors, H, W, 8.0, 0)
        arr = (_lib.DecodeLevel * 1)(lv)
        ptr = ctypes.cast(arr, ctypes.c_void_p) if levels else None
        return lib.mydet_decode_uv5_levels_f32(nlevels, ptr, 5 + C, 0, 5 + C, 5, 4, A, C, 1, 16, 16, bbox, cidx, score,
                                               A * H * W if N is None else N, None)
    bad = -1
    assert uv5(C=0) == bad and uv5(C=-1) == bad and uv5(C=129, ld=3 * 134 + 2) == bad
    assert uv5(A=0) == bad and uv5(A=17, ld=17 * 6 + 2) == bad
    assert uv5(bbox=None) == bad and uv5(cidx=None) == bad and uv5(score=None) == bad and uv5(box=None) == bad
    assert uv5(anchors=None) == bad                        # the layer has anchors
    assert uv5(ld=16) == bad                               # 3 anchors x 6 floats need 18 of a pixel
    assert uv5(ld=18) == bad                               # pitches are multiples of 4
    assert uv5(bbox=p + 4) == bad                          # 16-byte aligned base
    assert uv5(nlevels=6) == bad and uv5(nlevels=0) == bad and uv5(levels=False) == bad
    assert uv5(N=11) == bad                                # 3 x 2 x 2 candidates do not fit
    assert uv5(H=0) == bad

    def decode(mode):
        return lib.mydet_decode_f32(mode, p, 20, 6, 0, p, 20, 6, 5, 4, anch, 3, 1, 1, 2, 2, 8.0, 16, 16, p, p, p, 12, 0, None)
    assert decode(4) == bad and decode(5) == bad and decode(-1) == bad
    lv = _lib.DecodeLevel(p, 20, p, 20, anch_p, 2, 2, 8.0, 0)
    ptr = ctypes.cast((_lib.DecodeLevel * 1)(lv), ctypes.c_void_p)
    assert lib.mydet_decode_levels_f32(4, 1, ptr, 6, 0, 6, 5, 4, 3, 1, 1, 16, 16, p, p, p, 12, None) == bad
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'mydet.h')).read()
    assert 'MYDET_DECODE_UV5' not in header and '#define MYDET_ABI_VERSION 2 ' in header
    assert 'int mydet_decode_uv5_levels_f32(int nlevels, const mydet_decode_level *levels' in header


def test_ops_have_no_cpu_path():
    from mydetection_amd import ops
    x = torch.zeros(1, 20, 2, 2)                           # host tensors, with or without a GPU in the machine
    out = (torch.zeros(1, 12, 4), torch.zeros(1, 12, dtype=torch.int64), torch.zeros(1, 12))
    level = dict(box=x, ldbox=20, cls=x, ldcls=20, anchors_wh=[[1, 1]] * 3, H=2, W=2, stride=8, n_off=0)
    with pytest.raises(RuntimeError):
        ops.decode_uv5(x, 20, 6, 0, x, 20, 6, 5, 4, [[1, 1]] * 3, 3, 1, 1, 2, 2, 8, (16, 16), *out, 0)
    with pytest.raises(RuntimeError):
        ops.decode_uv5_levels([level], 6, 0, 6, 5, 4, 3, 1, 1, (16, 16), *out)
