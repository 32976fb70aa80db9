"""Fixtures of the Ultralytics (YOLOv5) decode layer and the ulo5m configuration, build container only.

    python tools/gen_golden_uv5.py                 # all of it
    python tools/gen_golden_uv5.py keys layer      # a subset: keys | layer | models

Imports the reference through oracle/_refimport.py and writes data only, under tests/golden/:
  uv5_keys.npz       the reference ulo5m model's state_dict key names + shapes and its inference cfg keys
  uv5_layer.npz      the reference's DetectLayer alone (models/detlayers/uv5.py:42-91) on seeded logits: n_cls 1 and 80, odd
                     maps, a quarter of the box logits drawn out to +-20 so that the ends of the parameterisation are reached
                     (cx -> -stride/2 and (g + 1.5) * stride, w -> 0 and 4 * anchor)
  ulo5m_b1_256.npz   the model on one synthetic image: every candidate, the class-probability gap of every candidate, the
  ulo5m_b1_640.npz   reference's detections at test.ap_conf_thres, 0.05 and test.default_conf_thres with their decision
                     margins and json rows; at 640^2 (25 200 candidates) the scores, class ids and gaps are complete and the
                     boxes a sample of 4 096, so the file stays small
The image seed of a model fixture is the one with the widest post-processing margin among the first few.  The synthetic
weights give few scores above the default 0.5: the 640^2 fixture records zero detections at that setting, the 256^2 one
(seed 4, the only one of its six seeds with any) 17, as they are.
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, 'tests', 'golden')

from oracle import _refimport, gen_golden  # noqa: E402
from mydetection_amd import synth  # noqa: E402

CONFIG = 'ulo5m'
LAYER_MAPS = ((5, 7), (13, 11))
MODELS = ((256, 6), (640, 3))
BIG_SAMPLES = 4096


def gen_keys():
    model, _ = _refimport.build_reference_model(CONFIG)
    sd = model.state_dict()
    keys = list(sd)
    inference = {k: v for k, v in _refimport.reference_config(CONFIG).items() if not k.startswith('train.')}
    np.savez_compressed(os.path.join(OUT, 'uv5_keys.npz'), **{
        f'{CONFIG}_keys': np.array(keys), f'{CONFIG}_shapes': np.array(json.dumps([list(sd[k].shape) for k in keys])),
        f'{CONFIG}_cfg': np.array(json.dumps(inference, sort_keys=True))})
    print(CONFIG, len(keys), 'keys')


def gen_layer():
    _refimport.install()
    with _refimport.no_pretrained():
        from models.detlayers.uv5 import DetectLayer
    out = {'maps': np.array(LAYER_MAPS, np.int64), 'strides': np.array([8, 16], np.int64)}
    B = 2
    for n_cls in (1, 80):
        cfg = _refimport.reference_config(CONFIG)
        cfg['model.fpn.out_strides'] = [8, 16, 32]
        cfg['general.num_class'] = n_cls
        for lvl, (h, w) in enumerate(LAYER_MAPS):
            layer = DetectLayer(lvl, cfg)
            A = layer.num_anchors
            key = f'c{n_cls}_{h}x{w}'
            t = synth._normal(f'uv5_layer.{key}.bbox', (B, A, h, w, 4), std=1.5)
            wide = synth._uniform(f'uv5_layer.{key}.where', t.shape, 0.0, 1.0) < 0.25
            t[wide] = synth._uniform(f'uv5_layer.{key}.wide', (int(wide.sum()),), -20.0, 20.0)
            conf = synth._normal(f'uv5_layer.{key}.conf', (B, A, h, w, 1), std=3.0)
            cls = synth._normal(f'uv5_layer.{key}.class', (B, A, h, w, n_cls), std=2.0)
            raw = {'bbox': torch.from_numpy(t), 'conf': torch.from_numpy(conf), 'class': torch.from_numpy(cls)}
            with torch.no_grad():
                preds, _ = layer(raw, (h * layer.stride, w * layer.stride))
            out[f'{key}_bbox_in'], out[f'{key}_conf_in'], out[f'{key}_class_in'] = t, conf, cls
            out[f'{key}_anchors'] = layer.anchors.numpy().astype(np.float32)
            out[f'{key}_bbox'] = preds['bbox'].numpy()
            out[f'{key}_class_idx'] = preds['class_idx'].numpy()
            out[f'{key}_score'] = preds['score'].numpy()
    np.savez_compressed(os.path.join(OUT, 'uv5_layer.npz'), **out)
    print('uv5_layer', len(out), 'arrays')


def gen_model(size, seeds):
    model, cfg = _refimport.build_reference_model(CONFIG)
    settings = (('ap', cfg['test.ap_conf_thres']), ('mid', 0.05), ('demo', cfg['test.default_conf_thres']))
    best = None
    for seed in range(seeds):
        with torch.no_grad():
            d = model(synth.make_images(1, size, seed=seed))[0]
        sc, ct = d.scores.numpy(), d.cats.numpy()
        m = min(gen_golden._margin(sc, ct, c) for _, c in settings)
        print(' ', CONFIG, size, 'seed', seed, 'margin', m, 'pass', [int((sc >= c).sum()) for _, c in settings])
        if best is None or m > best[0]:
            best = (m, seed)
    seed = best[1]
    x = synth.make_images(1, size, seed=seed)
    raws = []
    hook = model.rpn.register_forward_hook(lambda _m, _i, o: raws.extend(o))
    with torch.no_grad():
        d = model(x)[0]
    hook.remove()
    out = {'batch': 1, 'size': size, 'image_seed': seed, 'config': np.array(CONFIG)}
    boxes = d.bboxes.numpy()
    out['scores_0'], out['cats_0'] = d.scores.numpy(), d.cats.numpy()
    if boxes.shape[0] > 3 * BIG_SAMPLES:
        rng = np.random.Generator(np.random.PCG64(7))
        idx = np.sort(rng.choice(boxes.shape[0], BIG_SAMPLES, replace=False))
        out['bboxes_0_idx'], out['bboxes_0_val'], out['n_candidates'] = idx, boxes[idx], np.int64(boxes.shape[0])
    else:
        out['bboxes_0'] = boxes
    top2 = torch.cat([torch.sigmoid(r['class']).reshape(1, -1, r['class'].shape[-1]) for r in raws], 1).topk(2, -1).values
    out['cls_margin_0'] = (top2[..., 0] - top2[..., 1])[0].numpy()
    for tag, conf in settings:
        with torch.no_grad():
            r = model(x)[0].post_process(conf_thres=conf, nms_thres=cfg['test.nms_thres'])
        out[f'pp_{tag}_conf'], out[f'pp_{tag}_nms'] = np.float64(conf), np.float64(cfg['test.nms_thres'])
        out[f'pp_{tag}_bboxes_0'], out[f'pp_{tag}_cats_0'] = r.bboxes.numpy().reshape(-1, 4), r.cats.numpy()
        out[f'pp_{tag}_scores_0'] = r.scores.numpy()
        out[f'pp_{tag}_margin'] = np.float64(gen_golden._margin(out['scores_0'], out['cats_0'], conf))
        out[f'pp_{tag}_json_0'] = np.array(json.dumps(r.to_json(7)))
    fname = f'{CONFIG}_b1_{size}'
    np.savez_compressed(os.path.join(OUT, fname + '.npz'), **out)
    print(fname, 'seed', seed, 'N', out['scores_0'].size, 'dets', {t: out[f'pp_{t}_cats_0'].size for t, _ in settings},
          'pass', {t: int((out['scores_0'] >= c).sum()) for t, c in settings},
          'margin', {t: float(out[f'pp_{t}_margin']) for t, _ in settings},
          'cx min', float(boxes[:, 0].min()), 'bytes', os.path.getsize(os.path.join(OUT, fname + '.npz')))


if __name__ == '__main__':
    os.makedirs(OUT, exist_ok=True)
    torch.set_num_threads(int(os.environ.get('GEN_THREADS', '8')))
    which = sys.argv[1:] or ['keys', 'layer', 'models']
    if 'keys' in which:
        gen_keys()
    if 'layer' in which:
        gen_layer()
    if 'models' in which:
        for size, seeds in MODELS:
            gen_model(size, seeds)
