"""Scoring detections against ground truth on the device (reference: utils/evaluation/): `coco` for axis-aligned COCO-style
sets, `cepdof` for rotated CEPDOF-style sets.  Both are one evaluator, BboxEval (include/mydet.h: mydet_eval_*)."""
from .coco import BboxEval, coco_evaluate_bbox, myCOCOeval  # noqa: F401
from .cepdof import CEPDOFeval, evaluate_json  # noqa: F401
from .mot import MOTeval  # noqa: F401
