"""`Evaluator`: scores what the Detector returns against ground truth without going through JSON."""
import numpy as np

from .. import ops
from ..utils.constants import COCO_CATEGORY_IDS
from ..utils.evaluation.coco import BboxEval, _loaded


class Evaluator:
    """Collects detections and scores them on the device (include/mydet.h: mydet_eval_*).

    gt: a path or a loaded ground-truth dict.  kind: 'coco' (boxes x, y, w, h) or 'cepdof' (rotated boxes cx, cy, w, h, degrees).
    catIdx2id: class index -> category id, as in ImageObjects.to_json (None: the COCO ids).
    add(objects, img_ids) takes the ImageObjects of any predict_* / predict_frames* call; the boxes go through the arithmetic of
    to_json, (double)cx - (double)w/2, so the result equals the JSON route bit for bit.  add_json(rows) takes JSON rows.
    result() -> {'stats', 'summary', 'precision', 'recall', 'scores'}."""

    def __init__(self, gt, kind='coco', catIdx2id=None, device=None):
        self.rotated = ops._eval_kind(kind)
        self.kind, self.gt, self.device = kind, _loaded(gt), device
        self.cat_table = COCO_CATEGORY_IDS if catIdx2id is None else catIdx2id
        self.reset()

    def reset(self):
        self._img, self._cat, self._box, self._score, self._area = [], [], [], [], []

    def __len__(self):
        return len(self._img)

    def add(self, objects, img_ids):
        if not isinstance(objects, (list, tuple)):
            objects, img_ids = [objects], [img_ids]
        if len(objects) != len(img_ids):
            raise ValueError(f'Evaluator.add: {len(objects)} ImageObjects and {len(img_ids)} image ids')
        want = 'cxcywhd' if self.rotated else 'cxcywh'
        for o, img_id in zip(objects, img_ids):
            if o._bb_format != want:
                raise ValueError(f'Evaluator.add: kind {self.kind!r} scores {want} boxes, not {o._bb_format}')
            if o.scores is None:
                raise ValueError('Evaluator.add: detections without scores')
            b = o.bboxes.detach().cpu().numpy().astype(np.float64)
            if not self.rotated:
                b = np.stack([b[:, 0] - b[:, 2] / 2, b[:, 1] - b[:, 3] / 2, b[:, 2], b[:, 3]], axis=1)
            self._box.append(b)
            self._score.append(o.scores.detach().cpu().numpy().astype(np.float64))
            self._area.append(b[:, 2] * b[:, 3])
            self._cat += [self.cat_table[int(c)] for c in o.cats.cpu().tolist()]
            self._img += [img_id] * len(b)

    def add_json(self, rows):
        c = ops.eval_columns(rows, self.kind)
        self._img += c['image_id']
        self._cat += c['category_id']
        self._box.append(c['bbox'])
        self._score.append(c['score'])
        self._area.append(c['area'])

    def columns(self):
        width = 5 if self.rotated else 4
        return {'image_id': self._img, 'category_id': self._cat,
                'bbox': np.concatenate(self._box + [np.zeros((0, width))]), 'score': np.concatenate(self._score + [np.zeros(0)]),
                'area': np.concatenate(self._area + [np.zeros(0)])}

    def evaluator(self, **kwargs):
        """The BboxEval over what was added, before evaluate(): change its .params here."""
        e = BboxEval(self.gt, self.columns(), 'bbox', False, self.device, **kwargs)
        e.kind = self.kind
        return e

    def result(self):
        e = self.evaluator()
        e.evaluate()
        e.accumulate()
        e.summarize()
        return {'stats': e.stats, 'summary': e.summary, 'precision': e.eval['precision'], 'recall': e.eval['recall'],
                'scores': e.eval['scores']}
