"""`Evaluator` and `TrackEvaluator`: score what the Detector returns against ground truth without going through JSON."""
import numpy as np

from .. import ops
from ..utils.constants import COCO_CATEGORY_IDS
from ..utils.evaluation.coco import BboxEval, _loaded
from ..utils.evaluation.mot import MOTeval


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


class TrackEvaluator:
    """Collects tracked detections and scores them against ground-truth identities on the device (include/mydet.h: mydet_mot_*):
    the CLEAR MOT counts, MOTA, MOTP, MT / PT / ML, fragmentations, and IDF1 / IDP / IDR.

    gt: a path or a loaded ground-truth dict whose annotations carry an identity: the first of 'track_id' and 'person_id' present,
    or id_key.  kind: 'coco' (boxes x, y, w, h) or 'cepdof' (rotated boxes cx, cy, w, h, degrees).  iou_thrs: a pair is a
    possible match when its IoU is >= the threshold.  sequences: None groups the images by 'video_id' ordered by 'frame_id' when
    every image has both and otherwise makes one sequence in `images` order; a dict {name: [img_id, ...]} gives the sequences
    explicitly.  Frames without hypotheses or without ground truth count.  use_cats=False scores all categories as one.
    catIdx2id: class index -> category id, as in ImageObjects.to_json (None: the COCO ids).
    add(objects, img_ids) takes the ImageObjects of any tracked predict_frames* call (coasting=True output too) and raises
    ValueError when obj_ids is None; the boxes go through the arithmetic of to_json.  add_json(rows) takes rows with 'track_id'.
    result() -> {'iou_thrs', 'overall': [per threshold], 'sequences': {name: [per threshold]}, 'summary'}; every entry holds the
    integer counts (tp, fp, fn, idsw, frag, n_gt, n_hyp, idtp, idfp, idfn, n_ids, mt, pt, ml) and mota = 1 - (FN + FP + IDSW) / nGT,
    motp = SIOU / TP, precision, recall, idf1 = 2 IDTP / (nGT + nHyp), idp, idr.  motp is the MEAN IoU of the matches, not the
    distance of the CLEAR MOT paper: larger is better.  Every other ratio is one float64 division of exact integers.
    hota: False, True (alphas 0.05 .. 0.95) or a sequence of alphas, each > 0 and <= 1: result()['hota'] = {'alphas', 'overall',
    'sequences'} then holds HOTA, DetA, AssA, DetRe, DetPr, AssRe, AssPr and LocA per alpha and as means over the alphas
    (mydet_hota_*; units summed as the CLEAR rows are, not averaged over classes as TrackEval does), and the summary gains their
    table.  With hota=False the result is what it was."""

    def __init__(self, gt, kind='coco', iou_thrs=(0.5,), sequences=None, id_key=None, use_cats=True, catIdx2id=None, device=None,
                 hota=False):
        self.rotated = ops._eval_kind(kind)
        self.kind, self.gt, self.device = kind, _loaded(gt), device
        self.iou_thrs = ops._eval_thresholds(iou_thrs, 'iou_thrs')
        if not 1 <= len(self.iou_thrs) <= ops._lib.EVAL_MAX_THRS or np.isnan(self.iou_thrs).any():
            raise ValueError(f'TrackEvaluator: 1 to {ops._lib.EVAL_MAX_THRS} IoU thresholds expected, none of them NaN')
        if sequences is not None and not isinstance(sequences, dict):
            raise ValueError('TrackEvaluator: sequences is None or a dict {name: [img_id, ...]}')
        self.sequences, self.id_key, self.use_cats = sequences, id_key, bool(use_cats)
        self.hota = False if hota is False or hota is None else ops.hota_alphas(hota)
        ops.mot_sequences(self.gt, sequences)                        # the argument errors, before anything is added
        ops.mot_id_key(self.gt, id_key)
        self.cat_table = COCO_CATEGORY_IDS if catIdx2id is None else catIdx2id
        self.reset()

    def reset(self):
        self._img, self._cat, self._ids, self._box = [], [], [], []

    def __len__(self):
        return len(self._img)

    def add(self, objects, img_ids):
        if not isinstance(objects, (list, tuple)):
            objects, img_ids = [objects], [img_ids]
        if len(objects) != len(img_ids):
            raise ValueError(f'TrackEvaluator.add: {len(objects)} ImageObjects and {len(img_ids)} image ids')
        want = 'cxcywhd' if self.rotated else 'cxcywh'
        for o in objects:                                            # nothing is added unless everything can be
            if o._bb_format != want:
                raise ValueError(f'TrackEvaluator.add: kind {self.kind!r} scores {want} boxes, not {o._bb_format}')
            if o.obj_ids is None:
                raise ValueError('TrackEvaluator.add: objects without obj_ids (pass tracker= to the predict_frames* call)')
        for o, img_id in zip(objects, img_ids):
            b = o.bboxes.detach().cpu().numpy().astype(np.float64)
            if not self.rotated:
                b = np.stack([b[:, 0] - b[:, 2] / 2, b[:, 1] - b[:, 3] / 2, b[:, 2], b[:, 3]], axis=1)
            self._box.append(b)
            self._cat += [self.cat_table[int(c)] for c in o.cats.cpu().tolist()]
            self._ids += [int(i) for i in o.obj_ids.cpu().tolist()]
            self._img += [img_id] * len(b)

    def add_json(self, rows):
        c = ops.mot_columns(rows, self.kind)
        self._img += c['image_id']
        self._cat += c['category_id']
        self._ids += c['track_id']
        self._box.append(c['bbox'])

    def columns(self):
        width = 5 if self.rotated else 4
        return {'image_id': self._img, 'category_id': self._cat, 'track_id': self._ids,
                'bbox': np.concatenate(self._box + [np.zeros((0, width))])}

    def evaluator(self, **kwargs):
        """The MOTeval over what was added, before evaluate()."""
        return MOTeval(self.gt, self.columns(), self.kind, self.iou_thrs, self.sequences, self.id_key, self.use_cats, False, self.device,
                       hota=self.hota, **kwargs)

    def result(self):
        e = self.evaluator()
        e.evaluate()
        out = dict(e.summarize())
        out['summary'] = e.summary
        return out
