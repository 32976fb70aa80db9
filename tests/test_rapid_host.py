"""CPU tests of the RAPiD rotated-box models (configs rapid, rapid_psl1, yv3_pl1_80, u5m_rapid, d1_rapid): configuration and
state_dict against the reference's, a float64 restatement of RAPiDLayer pinned by fixtures made from the imported reference
(tools/gen_golden_rapid.py), the C ABI's argument checks and rotated-record layout, the synthetic recipe, and the multi-GPU
exchange of rotated records over gloo."""
import ctypes
import hashlib
import json
import os
import re

import numpy as np
import pytest
import torch

RAPID_CONFIGS = ('rapid', 'rapid_psl1', 'yv3_pl1_80', 'u5m_rapid', 'd1_rapid')


def rapid_f64(t, conf, cls, anchors, stride):
    """RAPiDLayer's inference branch (reference models/detlayers/rapid.py:36-81) in float64: raw logits t [B,A,H,W,5],
    conf [B,A,H,W,1], cls [B,A,H,W,C] -> (bbox [B,N,5] = cx, cy, w, h, deg; class_idx [B,N]; score [B,N])."""
    t, conf, cls = (np.asarray(a, np.float64) for a in (t, conf, cls))
    B, A, H, W, _ = t.shape
    sig = lambda v: 1.0 / (1.0 + np.exp(-v))
    gy, gx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing='ij')
    aw = np.asarray(anchors, np.float64)[:, 0].reshape(1, A, 1, 1)
    ah = np.asarray(anchors, np.float64)[:, 1].reshape(1, A, 1, 1)
    box = np.stack([(sig(t[..., 0]) + gx) * stride, (sig(t[..., 1]) + gy) * stride, np.exp(t[..., 2]) * aw,
                    np.exp(t[..., 3]) * ah, (sig(t[..., 4]) * 2 * np.pi - np.pi) / np.pi * 180], axis=-1)
    score = sig(conf[..., 0])
    if cls.shape[-1] > 0:
        p = sig(cls)
        idx = p.argmax(-1)
        score = np.sqrt(score * p.max(-1))
    else:
        idx = np.zeros(score.shape, np.int64)
    return box.reshape(B, -1, 5), idx.reshape(B, -1), score.reshape(B, -1)


@pytest.mark.parametrize('name', RAPID_CONFIGS)
def test_config_and_state_dict_match_the_reference(name, golden):
    from mydetection_amd import configs
    from mydetection_amd.models.general import name_to_model
    from mydetection_amd.models.detlayers.rapid import RAPiDLayer
    g = golden('rapid_keys')
    assert configs.get(name) == json.loads(str(g[f'{name}_cfg']))     # the reference file's inference keys, exactly
    m, cfg = name_to_model(name)
    sd = m.state_dict()
    assert list(sd) == [str(k) for k in g[f'{name}_keys']]
    assert [list(v.shape) for v in sd.values()] == json.loads(str(g[f'{name}_shapes']))
    assert all(type(d) is RAPiDLayer for d in m.det_layers) and len(m.det_layers) == 3
    assert m.bbox_param == 5 and m.bb_format == 'cxcywhd'


def test_rapid_layer_constructor():
    from mydetection_amd import configs
    from mydetection_amd.models.detlayers.rapid import RAPiDLayer
    cfg = configs.get('rapid')
    cfg['model.fpn.out_strides'] = [8, 16, 32]
    layer = RAPiDLayer(1, cfg)
    assert layer.num_anchors == 3 and layer.stride == 16 and layer.n_cls == 0
    assert layer.anchor_indices.tolist() == [3, 4, 5]
    np.testing.assert_array_equal(layer.anchors.numpy(), np.float32(cfg['model.rapid.anchors'][3:6]))
    assert layer.anch_00wha_all.shape == (9, 5)
    with pytest.raises(AssertionError):
        RAPiDLayer(0, dict(cfg, **{'model.angle.pred_range': 180}))
    with pytest.raises(NotImplementedError):
        layer({'bbox': torch.zeros(1, 3, 2, 2, 5)}, (32, 32), labels=[])


def test_float64_restatement_matches_the_reference_layer(golden):
    """Boxes and scores within float32 round-off of the reference; class ids equal where the class probabilities are apart;
    the angles, restated in float32 in the reference's operation order with pi as the float32 constant, equal the
    reference's bit for bit (this is what the decode kernel computes: csrc/decode.hip)."""
    g = golden('rapid_layer')
    n_wrap = 0
    for n_cls in (0, 80):
        for lvl, (h, w) in enumerate(g['maps']):
            key = f'c{n_cls}_{h}x{w}'
            t, conf, cls = g[f'{key}_bbox_in'], g[f'{key}_conf_in'], g[f'{key}_class_in']
            box, idx, score = rapid_f64(t, conf, cls, g[f'{key}_anchors'], float(g['strides'][lvl]))
            ref_box, ref_idx, ref_score = g[f'{key}_bbox'], g[f'{key}_class_idx'], g[f'{key}_score']
            assert box.shape == ref_box.shape == (2, 3 * h * w, 5)
            np.testing.assert_allclose(box[..., :4], ref_box[..., :4], rtol=1e-6, atol=1e-5)
            np.testing.assert_allclose(box[..., 4], ref_box[..., 4], rtol=0, atol=1e-4)
            np.testing.assert_allclose(score, ref_score, rtol=1e-6, atol=1e-7)
            if n_cls:
                p = np.sort(1 / (1 + np.exp(-cls.astype(np.float64))), -1).reshape(2, -1, n_cls)
                safe = p[..., -1] - p[..., -2] > 1e-6
                assert safe.mean() > 0.99
                np.testing.assert_array_equal(idx[safe], ref_idx[safe])
            else:
                assert not ref_idx.any()
            s = torch.sigmoid(torch.from_numpy(t[..., 4])).numpy()
            pi = np.float32(np.pi)
            deg32 = ((s * np.float32(2) * pi - pi) / pi * np.float32(180)).astype(np.float32)
            np.testing.assert_array_equal(deg32.reshape(2, -1), ref_box[..., 4])
            n_wrap += int((np.abs(ref_box[..., 4]) > 179.99).sum())
    assert n_wrap >= 20                                   # the fixture reaches the ends of the angle range


def test_abi_argument_checks():
    """The new decode mode and the rotated post-process entry points reject bad arguments before any launch."""
    from mydetection_amd import _lib
    lib = _lib.lib()
    buf = (ctypes.c_float * 256)()                        # host memory: every call below must fail before touching it
    p = ctypes.cast(buf, ctypes.c_void_p).value
    p = (p + 15) // 16 * 16
    anch = (ctypes.c_float * 32)(*([10.0] * 32))

    def decode(mode=3, A=3, C=0, box=p, bbox=p, cidx=p, score=p, anchors=anch, ld=20, H=2, W=2):
        return lib.mydet_decode_f32(mode, box, ld, 6 + C, 0, box, ld, 6 + C, 6, 5, anchors, A, C, 1, H, W, 8.0, 16, 16,
                                    bbox, cidx, score, A * H * W, 0, None)
    bad = -1
    assert decode(mode=4) == bad and decode(mode=-1) == bad
    assert decode(C=-1) == bad and decode(C=129, ld=3 * 135 + 3) == bad
    assert decode(mode=0, C=0) == bad                     # C == 0 is RAPiD's alone
    assert decode(A=17) == bad and decode(A=0) == bad
    assert decode(box=None) == bad and decode(bbox=None) == bad and decode(cidx=None) == bad and decode(score=None) == bad
    assert decode(anchors=None) == bad                   # RAPiD has anchors
    assert decode(ld=16) == bad                           # 3 anchors x 6 floats need 18 of a pixel
    assert decode(bbox=p + 4) == bad                      # 16-byte aligned base
    lv = _lib.DecodeLevel(p, 20, p, 20, ctypes.cast(anch, ctypes.c_void_p), 2, 2, 8.0, 0)
    arr = (_lib.DecodeLevel * 1)(lv)
    ptr = ctypes.cast(arr, ctypes.c_void_p)
    assert lib.mydet_decode_levels_f32(3, 6, ptr, 6, 0, 6, 6, 5, 3, 0, 1, 16, 16, p, p, p, 12, None) == bad    # > 5 levels
    assert lib.mydet_decode_levels_f32(3, 1, None, 6, 0, 6, 6, 5, 3, 0, 1, 16, 16, p, p, p, 12, None) == bad
    assert lib.mydet_decode_levels_f32(3, 1, ptr, 6, 0, 6, 6, 5, 3, 0, 1, 16, 16, p, p, p, 11, None) == bad   # N too small
    null = ctypes.c_void_p(0)
    assert lib.mydet_postprocess_rot_f32(null, null, null, 1, 1 << 20, 0.5, 0.5, 512, null, null, null, null, null, null,
                                         null) == -2
    assert lib.mydet_postprocess_rot_f32(p, p, p, 1, 100, 0.5, 0.5, 513, p, p, p, p, p, p, null) == bad
    assert lib.mydet_postprocess_rot_f32(p, p, p, 0, 100, 0.5, 0.5, 512, p, p, p, p, p, p, null) == bad
    assert lib.mydet_postprocess_rot_f32(null, p, p, 1, 100, 0.5, 0.5, 512, p, p, p, p, p, p, null) == bad
    assert lib.mydet_postprocess_rot_f32(p, p, p, 1, 100, 0.5, 0.5, 512, null, p, p, p, p, p, null) == bad
    assert lib.mydet_postprocess_records_rot_f32(p, p, p, 1, 100, 0.5, 0.5, null, p, null) == bad
    assert lib.mydet_postprocess_records_rot_f32(p, p, p, 1, 100, 0.5, 0.5, p + 4, p, null) == bad
    assert lib.mydet_postprocess_records_rot_f32(p, p, p, 1, 1 << 20, 0.5, 0.5, p, p, null) == -2
    assert lib.mydet_postprocess_records_rot_f32(null, p, p, 1, 100, 0.5, 0.5, p, p, null) == bad


def test_rotated_record_layout_from_the_header():
    from mydetection_amd import _lib, ops
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, 'include', 'mydet.h')).read()
    assert '#define MYDET_DECODE_RAPID  3' in header and ops.DECODE_RAPID == 3
    words = {m.group(1): m.group(2).strip() for m in re.finditer(r'#define MYDET_REC_(\w+)\s+(.+)', header)}
    assert words['ANGLE'] == 'MYDET_REC_WORDS' and words['ROT_WORDS'] == '(MYDET_REC_WORDS + MYDET_REC_TOPK)'
    assert _lib.REC_WORDS == 4100 and _lib.REC_ANGLE == 4100 and _lib.REC_ROT_WORDS == 4612
    assert _lib.REC_ROT_WORDS * 4 == 18448 and _lib.REC_ROT_WORDS % 4 == 0           # rows stay 16-byte aligned
    assert ops.record_words(4) == _lib.REC_WORDS and ops.record_words(5) == _lib.REC_ROT_WORDS
    with pytest.raises(ValueError):
        ops.record_words(6)
    rec = torch.arange(2 * _lib.REC_ROT_WORDS, dtype=torch.int32).view(2, -1)
    v = ops.record_views(rec)
    plain = ops.record_views(rec[:, :_lib.REC_WORDS].contiguous())
    for k in ('count', 'bbox', 'score', 'class_idx', 'index'):                        # every field at its 4-column offset
        assert torch.equal(v[k], plain[k]), k
    assert 'angle' not in plain and v['angle'].shape == (2, 512)
    assert v['angle'].view(torch.int32)[1, 0] == _lib.REC_ROT_WORDS + _lib.REC_ANGLE
    assert v['bbox'].stride() == (_lib.REC_ROT_WORDS, 4, 1)                         # the batched to_original kernel's layout
    boxes = ops.record_boxes(v, 1, 3)
    assert boxes.shape == (3, 5) and torch.equal(boxes[:, 4], v['angle'][1, :3]) and torch.equal(boxes[:, :4], v['bbox'][1, :3])


def test_rotated_json_needs_no_device():
    from mydetection_amd.utils.structures import ImageObjects
    b = torch.tensor([[10.5, 20.25, 30.0, 40.0, -179.5], [1.0, 2.0, 3.0, 4.0, 90.0]])
    d = ImageObjects(b, torch.tensor([0, 0]), None, torch.tensor([0.75, 0.5]), 'cxcywhd', (64, 64))
    js = d.to_json(3, eval_type='cxcywhd')
    assert js == [{'image_id': 3, 'category_id': 1, 'bbox': [10.5, 20.25, 30.0, 40.0, -179.5], 'score': 0.75},
                  {'image_id': 3, 'category_id': 1, 'bbox': [1.0, 2.0, 3.0, 4.0, 90.0], 'score': 0.5}]
    assert all(type(v) is float for r in js for v in r['bbox'])
    assert d.to_json('x', eval_type='cxcywhd', catIdx2id={0: 'person'})[0]['category_id'] == 'person'


# sha256 (first 16 hex digits) of make_state_dict of every configuration that existed before the RAPiD models, over (key,
# bytes) in state_dict order, both recipes for the EfficientNet-based ones: the RAPiD recipe changed none of them
EXISTING_STATE_DICTS = {
    'yolov3_80': 'cea47b91e8ca12eb', 'efficientdet-d1': 'ec96b3877d4f68a7', 'd1_fcs2_atss': 'b97b479e560e67a7',
    'd1_fcs2': 'b97b479e560e67a7', 'd1_fcs': '435e8b713fac6332', 'd1_fcs2s': '033f9a07d731605e',
    'd1_fcs2s_mos': '033f9a07d731605e', 'd1_fcs2_p3': '4fcc0afb5f3a3e92', 'd1_yv3': '1b2dbac5d06670cd',
    'u5m_yv3': 'd1b16662b688d3e8', 'u5m_fcs2': '01fe5f8c093a213f'}


def _state_dict_hash(name):
    from mydetection_amd import synth
    from mydetection_amd.models.general import load_config, state_dict_template
    cfg = load_config(name)
    h = hashlib.sha256()
    tpl = state_dict_template(name)
    for recipe in ('conditioned', 'stiff') if 'efficientnet' in str(cfg.get('model.backbone.name')) else ('conditioned',):
        for k, v in synth.make_state_dict(tpl, name, recipe).items():
            h.update(k.encode())
            h.update(v.numpy().tobytes())
    return h.hexdigest()[:16]


def test_synthetic_weights_of_existing_configs_unchanged():
    for name, want in EXISTING_STATE_DICTS.items():
        assert _state_dict_hash(name) == want, name


def test_rapid_synthetic_recipe():
    """Deterministic (a pure function of the keys), the angle rows wide enough to spread sigmoid(t_angle) over (0, 1), the
    objectness far below zero; d1_rapid finds its calibration (the fixture) through synth.load_calibration's fallback."""
    from mydetection_amd import synth
    from mydetection_amd.models.general import state_dict_template
    tpl = state_dict_template('rapid')
    a, b = synth.make_state_dict(tpl, 'rapid'), synth.make_state_dict(tpl, 'rapid')
    assert all(torch.equal(a[k], b[k]) for k in a)
    bias = a['rpn.heads.conv_0.bias'].numpy().reshape(3, 6)
    assert np.all(np.abs(bias[:, :5]) < 0.3) and np.all(bias[:, 5] < -5.0)
    w = a['rpn.heads.conv_1.weight'].numpy().reshape(3, 6, -1)
    assert np.all(w[:, 4].std(-1) > 2.5 * w[:, 2].std(-1))          # angle logits wider than the log-size ones
    assert _state_dict_hash('rapid') == _state_dict_hash('rapid_psl1')           # the same network
    calib = synth.load_calibration('d1_rapid')
    assert '__std__/rpn.bbox_nets.2.3' in calib and '__std__/rpn.class_nets.0.3' in calib
    std, bias = synth._efdet_row_targets('bbox', 15)
    assert std[4] == std[9] == std[14] == synth._RAPID_TARGETS['angle'][0]
    std, bias = synth._efdet_row_targets('class', 3)
    assert np.all(bias == synth._RAPID_TARGETS['conf'][1])


def _worker(rank, world, port, total, q):
    import torch.distributed as dist
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    from mydetection_amd import parallel
    g = torch.Generator().manual_seed(7)
    glob = {'count': torch.randint(0, 513, (total,), generator=g, dtype=torch.int32),
            'bbox': torch.rand(total, 512, 4, generator=g), 'class_idx': torch.zeros(total, 512, dtype=torch.int64),
            'score': torch.rand(total, 512, generator=g), 'index': torch.randint(0, 64512, (total, 512), generator=g, dtype=torch.int32),
            'angle': torch.rand(total, 512, generator=g) * 360 - 180}
    lo, hi = parallel.shard_range(total, rank, world)
    allrec = parallel.gather_detections({k: v[lo:hi].clone() for k, v in glob.items()}, total=total)
    ok = tuple(allrec['records'].shape) == (total, parallel._lib.REC_ROT_WORDS)
    for k in glob:
        ok = ok and torch.equal(allrec[k], glob[k])
    objs = parallel.records_to_objects(allrec, img_hw=(1024, 1024), bb_format='cxcywhd')
    ok = ok and all(o.bboxes.shape == (int(c), 5) and torch.equal(o.bboxes[:, 4], glob['angle'][b, :int(c)])
                    for b, (o, c) in enumerate(zip(objs, glob['count'])))
    q.put((rank, bool(ok)))
    dist.destroy_process_group()


def test_gloo_world2_gathers_rotated_records():
    import socket
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, 5, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=120) for _ in procs)
    for p in procs:
        p.join(timeout=60)
    assert res == {0: True, 1: True}
