"""COCO bbox evaluation on the device (reference: utils/evaluation/coco.py, which subclasses pycocotools' COCOeval).

Same call shapes: coco_evaluate_bbox(dts_json, gt_json) -> (summary, ap, ap50, ap75), and a myCOCOeval with evaluate(),
accumulate(), summarize(), .params, .stats, .summary, .eval and .ious.  The work is three HIP launches on the packed arrays
(include/mydet.h: mydet_eval_ious_f64, mydet_eval_match_f64, mydet_eval_accumulate_f64, where the rules are written down); the
packing before them and the 12-number summary after them are host numpy (ops.eval_pack, ops.eval_summarize).  pycocotools is
not used, so bit-identity with it is not claimed: the claim is equality with the documented rules.
"""
import collections.abc
import copy
import datetime
import json

import numpy as np

from ... import ops


def _loaded(obj):
    if isinstance(obj, str):
        with open(obj, 'r') as f:
            return json.load(f)
    return obj


class _GroupIous(collections.abc.Mapping):
    """pycocotools' `ious`: (image id, category id) -> float64 [detections, ground truths] in the group's packed order, or []
    for a group that holds neither.  Cut out of the one IoU buffer on demand; the buffer is copied to the host once."""

    def __init__(self, pack, buffer):
        self._pack, self._buffer, self._host = pack, buffer, None
        self._img = {v: n for n, v in enumerate(pack['img_ids'])}
        self._cat = {v: n for n, v in enumerate(pack['cat_ids'])}

    def __len__(self):
        return self._pack['I'] * self._pack['K']

    def __iter__(self):
        return ((i, k) for i in self._pack['img_ids'] for k in self._pack['cat_ids'])

    def __getitem__(self, key):
        p = self._pack
        g = self._cat[key[1]] * p['I'] + self._img[key[0]]
        nd, ng = int(p['dt_start'][g + 1] - p['dt_start'][g]), int(p['gt_start'][g + 1] - p['gt_start'][g])
        if nd == 0 and ng == 0:
            return []
        if self._host is None:
            self._host = self._buffer.cpu().numpy()
        c = int(np.searchsorted(p['groups'], g))
        return self._host[p['pair_start'][c]:p['pair_start'][c + 1]].reshape(nd, ng)


class BboxEval:
    """The evaluator behind myCOCOeval (kind 'coco') and CEPDOFeval (kind 'cepdof').  dt_json: a path, JSON rows, or the columns
    of ops.eval_columns.  gt_json: a path or a loaded dict.  Images and categories are those of the ground truth; params.iouThrs,
    recThrs, maxDets and areaRng may be changed before evaluate().  keep_rows: also keep the matched ground-truth row of every
    detection at every (area range, threshold) in .matches['gt_row']."""
    kind = 'coco'

    def __init__(self, gt_json, dt_json, iouType='bbox', str_print=False, device=None, keep_rows=False):
        if iouType != 'bbox':
            raise NotImplementedError(f'iouType {iouType!r}: bbox evaluation only')
        self.str_print = str_print
        self.gt_json, self.dt_json = _loaded(gt_json), _loaded(dt_json)
        self.device, self.keep_rows = device, keep_rows
        self.params = ops.EvalParams()
        self.params.imgIds = sorted(im['id'] for im in self.gt_json['images'])
        self.params.catIds = sorted(c['id'] for c in self.gt_json['categories'])
        self._paramsEval = {}
        self.eval, self.stats, self.summary, self.ious, self.matches = {}, [], '', {}, {}
        self.packed = None

    def _say(self, text):
        if self.str_print:
            print(text)

    def evaluate(self):
        """Pack on the host, then IoU and matching on the device (two launches, no synchronisation)."""
        self._say('Running per image evaluation...')
        p = self.params
        p.imgIds, p.catIds, p.maxDets = list(np.unique(p.imgIds)), list(np.unique(p.catIds)), sorted(p.maxDets)
        pack = ops.eval_pack(self.dt_json, self.gt_json, self.kind, p.maxDets[-1])
        self.packed = ops.EvalSet(pack, self.device)
        buffer = ops.eval_ious(self.packed)
        matched, ignored, gt_row = ops.eval_match(self.packed, buffer, p.iouThrs, p.areaRng, rows=self.keep_rows)
        self.ious = _GroupIous(pack, buffer)
        self.matches = {'matched': matched, 'ignored': ignored, 'gt_row': gt_row, 'ious': buffer}
        self._paramsEval = copy.deepcopy(p)
        self.eval = {}

    def accumulate(self, p=None):
        """One launch, then the three arrays come to the host: .eval as in the reference."""
        self._say('Accumulating evaluation results...')
        if not self.matches:
            raise Exception('Please run evaluate() first')
        p = self.params if p is None else p
        pe = self._paramsEval
        precision, recall, scores = ops.eval_accumulate(self.packed, self.matches['matched'], self.matches['ignored'], len(pe.iouThrs),
                                                        pe.areaRng, p.maxDets, p.recThrs)
        self.eval = {'params': p, 'counts': [len(pe.iouThrs), len(p.recThrs), len(pe.catIds), len(pe.areaRng), len(p.maxDets)],
                     'date': datetime.datetime.now().strftime('%Y-%m-%d %H:%M:%S'),
                     'precision': precision.cpu().numpy(), 'recall': recall.cpu().numpy(), 'scores': scores.cpu().numpy()}

    def summarize(self):
        if not self.eval:
            raise Exception('Please run accumulate() first')
        self.stats, self.summary = ops.eval_summarize(self.eval['precision'], self.eval['recall'], self.params)
        self._say(self.summary)


class myCOCOeval(BboxEval):
    kind = 'coco'


def coco_evaluate_bbox(dts_json, gt_json, str_print=True):
    if str_print:
        print('Initialing validation set...')
    e = myCOCOeval(gt_json, dts_json, 'bbox', str_print)
    e.evaluate()
    e.accumulate()
    e.summarize()
    return e.summary, e.stats[0], e.stats[1], e.stats[2]
