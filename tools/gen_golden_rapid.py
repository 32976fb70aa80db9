"""Fixtures of the RAPiD rotated-box models (configs rapid, rapid_psl1, yv3_pl1_80, u5m_rapid, d1_rapid), build container only.

    python tools/gen_golden_rapid.py                 # all of it
    python tools/gen_golden_rapid.py keys layer      # a subset: calib | keys | layer | models

Imports the reference through oracle/_refimport.py (build_reference_model under no_pretrained: the EfficientNet download is
never reached) and writes data only, under tests/golden/:
  d1_rapid.calib.npz    BatchNorm running statistics + final-layer spreads of d1_rapid (oracle.calibrate_bn.calibrate;
                        synth.load_calibration reads it from here)
  rapid_keys.npz        per configuration: the reference model's state_dict key names + shapes and its inference cfg keys
  rapid_layer.npz       the reference's RAPiDLayer alone (models/detlayers/rapid.py:36-81) on seeded logits: n_cls 0 and 80,
                        odd maps, angle logits out to +-17 (angles within float32 round-off of +-180)
  rapid_b1_256.npz      the model on one synthetic image: every candidate, the class-probability gap of every candidate
  d1_rapid_b1_256.npz   (n_cls > 0 only), the reference's detections at test.ap_conf_thres, 0.05 and test.default_conf_thres
  rapid_b1_1024.npz     with their decision margins; at 1024^2 (64 512 candidates) the scores are complete and the boxes a
                        sample, so the file stays small
The image seed of a model fixture is the one with the widest post-processing margin among the first few.
"""
import json
import os
import shutil
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, 'tests', 'golden')

from oracle import _refimport, calibrate_bn, gen_golden  # noqa: E402
from mydetection_amd import synth  # noqa: E402

CONFIGS = ('rapid', 'rapid_psl1', 'yv3_pl1_80', 'u5m_rapid', 'd1_rapid')
LAYER_MAPS = ((5, 7), (13, 11))
MODELS = (('rapid', 256, 6), ('d1_rapid', 256, 6), ('rapid', 1024, 3))
BIG_SAMPLES = 4096


def gen_calib():
    calibrate_bn.calibrate('d1_rapid')
    shutil.move(os.path.join(ROOT, 'mydetection_amd', 'calib', 'd1_rapid.npz'), os.path.join(OUT, 'd1_rapid.calib.npz'))
    synth._CALIB_CACHE.clear()


def gen_keys():
    out = {}
    for name in CONFIGS:
        model, _ = _refimport.build_reference_model(name)
        sd = model.state_dict()
        keys = list(sd)
        inference = {k: v for k, v in _refimport.reference_config(name).items() if not k.startswith('train.')}
        out[f'{name}_keys'] = np.array(keys)
        out[f'{name}_shapes'] = np.array(json.dumps([list(sd[k].shape) for k in keys]))
        out[f'{name}_cfg'] = np.array(json.dumps(inference, sort_keys=True))
        print(name, len(keys), 'keys')
    np.savez_compressed(os.path.join(OUT, 'rapid_keys.npz'), **out)


def gen_layer():
    _refimport.install()
    with _refimport.no_pretrained():
        from models.detlayers.rapid import RAPiDLayer
    out = {'maps': np.array(LAYER_MAPS, np.int64), 'strides': np.array([8, 16], np.int64)}
    B = 2
    for n_cls, base in ((0, 'rapid'), (80, 'yv3_pl1_80')):
        cfg = _refimport.reference_config(base)
        cfg['model.fpn.out_strides'] = [8, 16, 32]
        for lvl, (h, w) in enumerate(LAYER_MAPS):
            layer = RAPiDLayer(lvl, cfg)
            A = layer.num_anchors
            key = f'c{n_cls}_{h}x{w}'
            t = synth._normal(f'rapid_layer.{key}.bbox', (B, A, h, w, 5), std=1.5)
            ang = t[..., 4].reshape(-1)
            ang[: ang.size // 4] = synth._uniform(f'rapid_layer.{key}.angle', (ang.size // 4,), -17.0, 17.0)
            t[..., 4] = ang.reshape(t[..., 4].shape)
            conf = synth._normal(f'rapid_layer.{key}.conf', (B, A, h, w, 1), std=3.0)
            cls = synth._normal(f'rapid_layer.{key}.class', (B, A, h, w, n_cls), std=2.0)
            raw = {'bbox': torch.from_numpy(t), 'conf': torch.from_numpy(conf), 'class': torch.from_numpy(cls)}
            with torch.no_grad():
                preds, _ = layer(raw, (h * layer.stride, w * layer.stride))
            out[f'{key}_bbox_in'], out[f'{key}_conf_in'], out[f'{key}_class_in'] = t, conf, cls
            out[f'{key}_anchors'] = layer.anchors.numpy().astype(np.float32)
            out[f'{key}_bbox'] = preds['bbox'].numpy()
            out[f'{key}_class_idx'] = preds['class_idx'].numpy()
            out[f'{key}_score'] = preds['score'].numpy()
    np.savez_compressed(os.path.join(OUT, 'rapid_layer.npz'), **out)
    print('rapid_layer', len(out), 'arrays')


def _images(cfg, size, seed):
    x = synth.make_images(1, size, seed=seed)
    return (x - gen_golden.MEAN) / gen_golden.STD if cfg['general.input_format'] == 'RGB_1_norm' else x


def gen_model(name, size, seeds):
    model, cfg = _refimport.build_reference_model(name)
    settings = (('ap', cfg['test.ap_conf_thres']), ('mid', 0.05), ('demo', cfg['test.default_conf_thres']))
    best = None
    for seed in range(seeds):
        with torch.no_grad():
            d = model(_images(cfg, size, seed))[0]
        sc, ct = d.scores.numpy(), d.cats.numpy()
        m = min(gen_golden._margin(sc, ct, c) for _, c in settings)
        print(' ', name, size, 'seed', seed, 'margin', m, 'pass', [int((sc >= c).sum()) for _, c in settings])
        if best is None or m > best[0]:
            best = (m, seed)
    seed = best[1]
    x = _images(cfg, size, seed)
    with torch.no_grad():
        d = model(x)[0]
    out = {'batch': 1, 'size': size, 'image_seed': seed, 'config': np.array(name)}
    boxes = d.bboxes.numpy()
    out['scores_0'], out['cats_0'] = d.scores.numpy(), d.cats.numpy()
    if boxes.shape[0] > 3 * BIG_SAMPLES:
        rng = np.random.Generator(np.random.PCG64(7))
        idx = np.sort(rng.choice(boxes.shape[0], BIG_SAMPLES, replace=False))
        out['bboxes_0_idx'], out['bboxes_0_val'], out['n_candidates'] = idx, boxes[idx], np.int64(boxes.shape[0])
    else:
        out['bboxes_0'] = boxes
    if cfg['general.num_class'] > 0:
        raws = []
        model.rpn.register_forward_hook(lambda _m, _i, o: raws.extend(o))
        with torch.no_grad():
            model(x)
        top2 = torch.cat([torch.sigmoid(r['class']).reshape(1, -1, r['class'].shape[-1]) for r in raws], 1).topk(2, -1).values
        out['cls_margin_0'] = (top2[..., 0] - top2[..., 1])[0].numpy()
    for tag, conf in settings:
        with torch.no_grad():
            r = model(x)[0].post_process(conf_thres=conf, nms_thres=cfg['test.nms_thres'])
        out[f'pp_{tag}_conf'], out[f'pp_{tag}_nms'] = np.float64(conf), np.float64(cfg['test.nms_thres'])
        out[f'pp_{tag}_bboxes_0'], out[f'pp_{tag}_cats_0'] = r.bboxes.numpy(), r.cats.numpy()
        out[f'pp_{tag}_scores_0'] = r.scores.numpy()
        out[f'pp_{tag}_margin'] = np.float64(gen_golden._margin(out['scores_0'], out['cats_0'], conf))
        out[f'pp_{tag}_json_0'] = np.array(json.dumps(r.to_json(7, eval_type='cxcywhd')))
    fname = f'{name}_b1_{size}'
    np.savez_compressed(os.path.join(OUT, fname + '.npz'), **out)
    print(fname, 'seed', seed, 'N', out['scores_0'].size, 'dets', {t: out[f'pp_{t}_cats_0'].size for t, _ in settings},
          'pass', {t: int((out['scores_0'] >= c).sum()) for t, c in settings},
          'margin', {t: float(out[f'pp_{t}_margin']) for t, _ in settings},
          'angle range', (float(boxes[:, 4].min()), float(boxes[:, 4].max())))


if __name__ == '__main__':
    os.makedirs(OUT, exist_ok=True)
    torch.set_num_threads(int(os.environ.get('GEN_THREADS', '8')))
    which = sys.argv[1:] or ['calib', 'keys', 'layer', 'models']
    only = os.environ.get('RAPID_MODELS')              # e.g. RAPID_MODELS=rapid: the fixtures of one configuration
    if 'calib' in which:
        gen_calib()
    if 'keys' in which:
        gen_keys()
    if 'layer' in which:
        gen_layer()
    if 'models' in which:
        for name, size, seeds in MODELS:
            if not only or name in only.split(','):
                gen_model(name, size, seeds)
