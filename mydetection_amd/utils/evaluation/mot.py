"""Track scoring on the device: the CLEAR MOT metrics (MOTA, MOTP, ID switches, fragmentations, MT / PT / ML) and the identity
metrics (IDF1, IDP, IDR).

The reference has no counterpart: it has no tracking loop.  Its CEPDOF / COSSY ground truth carries a `person_id` per box
(datasets/cossy/visualize_mot.py) and tracked calls return ImageObjects.obj_ids; this module is the scorer between them.  The
work is four HIP launches on the packed arrays (include/mydet.h: mydet_eval_ious_f64, mydet_mot_clear_f64, mydet_mot_id_overlap,
mydet_mot_id_assign, where the rules are written down); the packing before them and the ratios after them are host numpy
(ops.mot_pack, ops.mot_summarize).  py-motmetrics and TrackEval are not used, so agreement with them is not claimed: the claim is
equality with the documented rules.  `motp` is the mean IoU of the matched pairs, not a distance.

hota= adds HOTA (Luiten et al.): three more launches on the same packed arrays and the same IoUs (mydet_hota_align_f64,
mydet_hota_match, mydet_hota_score_f64), then ops.hota_summarize on the host.  Units are summed into sequence rows and one overall
row as the CLEAR rows are, which is not TrackEval's averaging over classes.
"""
from ... import ops
from .coco import _loaded


class MOTeval:
    """dt_json: a path, JSON rows that carry 'track_id', or the columns of ops.mot_columns.  gt_json: a path or a loaded dict whose
    annotations carry an identity ('track_id' or 'person_id', or id_key).  kind: 'coco' (boxes x, y, w, h) or 'cepdof' (rotated
    boxes cx, cy, w, h, degrees).  sequences: see ops.mot_sequences.  use_cats=False scores all categories as one.
    evaluate() packs and launches; summarize() brings the counts to the host: .result, .summary (text) and .raw (numpy).
    keep_rows: also keep the matched hypothesis row of every ground truth at every threshold in .raw['gt_match'].
    hota: False, True (alphas 0.05 .. 0.95) or a sequence of alphas, each > 0 and <= 1.  When it is on, result['hota'] =
    {'alphas', 'overall': entry, 'sequences': {name: entry}} (ops.hota_summarize), the HOTA table follows the CLEAR table in
    .summary, and .raw['hota'] holds the raw arrays; when it is off nothing changes."""

    def __init__(self, gt_json, dt_json, kind='coco', iou_thrs=(0.5,), sequences=None, id_key=None, use_cats=True, str_print=False,
                 device=None, keep_rows=False, hota=False):
        ops._eval_kind(kind)
        self.kind, self.gt_json, self.dt_json = kind, _loaded(gt_json), _loaded(dt_json)
        self.iou_thrs = ops._eval_thresholds(iou_thrs, 'iou_thrs')
        if len(self.iou_thrs) < 1:
            raise ValueError('MOTeval: at least one IoU threshold expected')
        self.sequences, self.id_key, self.use_cats = sequences, id_key, bool(use_cats)
        self.str_print, self.device, self.keep_rows = str_print, device, keep_rows
        self.hota_alphas = None if hota is False or hota is None else ops.hota_alphas(hota)
        self.packed, self.tensors, self.hota_tensors, self.raw, self.result, self.summary = None, {}, {}, {}, {}, ''

    def evaluate(self):
        """Pack on the host, then the four launches, and with hota= the three HOTA launches on the same IoUs (no synchronisation)."""
        pack = ops.mot_pack(self.dt_json, self.gt_json, self.kind, self.sequences, self.id_key, self.use_cats)
        self.packed = ops.MotSet(pack, self.device)
        self.tensors = ops.mot_evaluate(self.packed, self.iou_thrs, rows=self.keep_rows)
        self.hota_tensors = {} if self.hota_alphas is None else ops.hota_evaluate(self.packed, self.hota_alphas, ious=self.tensors['ious'])
        self.raw, self.result, self.summary = {}, {}, ''

    def summarize(self):
        if not self.tensors:
            raise Exception('Please run evaluate() first')
        self.raw = {k: None if v is None else v.cpu().numpy() for k, v in self.tensors.items()}
        self.result, self.summary = ops.mot_summarize(self.raw, self.packed.pack, self.iou_thrs)
        if self.hota_alphas is not None:
            self.raw['hota'] = {k: v.cpu().numpy() for k, v in self.hota_tensors.items()}
            self.result['hota'], text = ops.hota_summarize(self.raw['hota'], self.packed.pack, self.hota_alphas)
            self.summary += text
        if self.str_print:
            print(self.summary)
        return self.result


def evaluate_json(dts_json, gt_json, kind='cepdof', iou_thrs=(0.5,), str_print=True, hota=False, **kwargs):
    """Hypothesis rows with 'track_id' against a ground truth with identities -> (summary text, MOTA, IDF1, ID switches): the
    overall numbers at the first threshold.  hota= (a keyword of MOTeval) appends the HOTA table to the summary text; the tuple
    stays as it is."""
    e = MOTeval(gt_json, dts_json, kind, iou_thrs, str_print=str_print, hota=hota, **kwargs)
    e.evaluate()
    e.summarize()
    first = e.result['overall'][0]
    return e.summary, first['mota'], first['idf1'], first['idsw']
