"""CEPDOF evaluation of rotated boxes on the device (reference: utils/evaluation/cepdof.py).

evaluate_json(dts_json, gt_json_path) -> (summary, ap, ap50, ap75) and CEPDOFeval with the call shape of the reference.  Boxes are
(cx, cy, w, h, degrees).  The IoU of a pair is the exact area of intersection in float32 (include/mydet.h:
mydet_rotated_iou_f32) where the reference rasterises both boxes into image-sized masks (iou_rle): the documented deviation of
the rotated NMS.  Matching, accumulation and summary are those of the COCO evaluator (coco.BboxEval).
"""
from .coco import BboxEval


class CEPDOFeval(BboxEval):
    kind = 'cepdof'

    def __init__(self, gt_json, dt_json, iouType='bbox', str_print=True, device=None, keep_rows=False):
        assert iouType == 'bbox', 'Only support (rotated) bbox iou type'
        super().__init__(gt_json, dt_json, iouType, str_print, device, keep_rows)


def evaluate_json(dts_json, gt_json_path):
    print('Initialing validation set...')
    e = CEPDOFeval(gt_json_path, dts_json, 'bbox')
    e.evaluate()
    e.accumulate()
    e.summarize()
    return e.summary, e.stats[0], e.stats[1], e.stats[2]
