"""Small named evaluation cases (test code).  Each isolates one rule of include/mydet.h "Scoring detections against ground
truth"; tests/test_eval_host.py asserts on the restatement that the rule really fires in its case, tests/test_gpu_eval.py holds
the device to the restatement on all of them.  A case is (ground-truth dict, detection rows, parameter overrides or None); all are
axis-aligned ('coco').  Coordinates are multiples of 1/4, so areas and IoUs such as 0.5 and 0.75 are exact."""
import numpy as np


def gt_set(n_images, n_cats, anns):
    return {'images': [{'id': 10 * (i + 1), 'height': 480, 'width': 640} for i in range(n_images)],
            'categories': [{'id': k + 1} for k in range(n_cats)], 'annotations': anns}


def ann(img, cat, box, area=None, crowd=0):
    return {'image_id': 10 * (img + 1), 'category_id': cat + 1, 'bbox': [float(v) for v in box],
            'area': float(box[2] * box[3] if area is None else area), 'iscrowd': crowd}


def det(img, cat, box, score):
    return {'image_id': 10 * (img + 1), 'category_id': cat + 1, 'bbox': [float(v) for v in box], 'score': score}


def threshold_hit_exactly():
    # IoU 50/100 and 75/100: equal to the thresholds .5 and .75, which therefore match
    return gt_set(1, 2, [ann(0, 0, [0, 0, 10, 10]), ann(0, 1, [0, 0, 10, 10])]), [det(0, 0, [0, 0, 10, 5], .9), det(0, 1, [0, 0, 10, 7.5], .8)], None


def threshold_above_the_cap():
    # t = 1 is lowered to 1 - 1e-10: a perfect detection matches at it, one at IoU 0.99 does not
    return (gt_set(1, 1, [ann(0, 0, [0, 0, 10, 10]), ann(0, 0, [50, 50, 100, 100])]),
            [det(0, 0, [0, 0, 10, 10], .9), det(0, 0, [50, 50, 100, 99], .8)], {'iouThrs': np.array([.5, 1.0])})


def equal_iou_later_wins():
    return gt_set(1, 1, [ann(0, 0, [0, 0, 10, 10]), ann(0, 0, [0, 0, 10, 10])]), [det(0, 0, [0, 0, 10, 10], .9), det(0, 0, [0, 0, 10, 10], .8),
                                                                                  det(0, 0, [0, 0, 10, 10], .7)], None


def crowd_matched_by_several():
    # three detections inside a crowd region (IoU i/da = 1), one on an ordinary ground truth
    return (gt_set(1, 1, [ann(0, 0, [0, 0, 200, 200], crowd=1), ann(0, 0, [300, 300, 40, 40])]),
            [det(0, 0, [10, 10, 20, 20], .9), det(0, 0, [50, 50, 20, 30], .8), det(0, 0, [100, 100, 40, 20], .7), det(0, 0, [300, 300, 40, 40], .6),
             det(0, 0, [180, 180, 40, 40], .5)], None)


def non_ignored_match_stops_the_walk():
    # range 'small': the 40 x 40 ground truth (IoU .81 with the detection) is ignored, the 30 x 30 one (IoU .69) is not
    return gt_set(1, 1, [ann(0, 0, [0, 0, 40, 40]), ann(0, 0, [0, 0, 30, 30])]), [det(0, 0, [0, 0, 36, 36], .9)], None


def ignored_match_stays():
    # annotation order: the large (ignored in 'small') ground truth first, IoU .81; the small one second, IoU .5625
    return gt_set(1, 1, [ann(0, 0, [0, 0, 40, 40]), ann(0, 0, [0, 0, 27, 27])]), [det(0, 0, [0, 0, 36, 36], .9)], None


def ground_truth_outside_each_range():
    boxes = ([0, 0, 20, 25], [100, 0, 50, 100], [200, 200, 200, 100], [0, 300, 32, 32], [100, 300, 96, 96])
    return gt_set(1, 1, [ann(0, 0, b) for b in boxes]), [det(0, 0, b, .9 - .1 * n) for n, b in enumerate(boxes)], None


def unmatched_detection_outside_the_range():
    return (gt_set(1, 1, [ann(0, 0, [0, 0, 20, 25])]),
            [det(0, 0, [300, 300, 10, 10], .9), det(0, 0, [100, 100, 50, 50], .8), det(0, 0, [200, 0, 100, 100], .7), det(0, 0, [0, 0, 20, 25], .6)], None)


def boxes_that_only_touch():
    return gt_set(1, 1, [ann(0, 0, [0, 0, 10, 10])]), [det(0, 0, [10, 0, 10, 10], .9), det(0, 0, [0, 10, 10, 10], .8), det(0, 0, [10, 10, 5, 5], .7)], None


def zero_area_boxes():
    return (gt_set(1, 1, [ann(0, 0, [0, 0, 10, 10]), ann(0, 0, [20, 20, 0, 0])]),
            [det(0, 0, [5, 5, 0, 10], .9), det(0, 0, [20, 20, 0, 0], .8), det(0, 0, [0, 0, 10, 10], .7)], None)


def more_detections_than_max_dets():
    # 105 detections in one group: the five lowest scores (one of them the only true positive of the second box) are cut
    dts = [det(0, 0, [400, 400, 8, 8], .5 + .004 * n) for n in range(103)]
    dts += [det(0, 0, [0, 0, 10, 10], .95), det(0, 0, [50, 50, 10, 10], .4)]
    return gt_set(1, 1, [ann(0, 0, [0, 0, 10, 10]), ann(0, 0, [50, 50, 10, 10])]), dts, None


def one_sided_groups():
    # image 0 holds ground truth only, image 1 detections only, image 2 both
    return (gt_set(3, 1, [ann(0, 0, [0, 0, 10, 10]), ann(2, 0, [0, 0, 10, 10])]),
            [det(1, 0, [0, 0, 10, 10], .9), det(2, 0, [0, 0, 10, 10], .8)], None)


def category_without_ground_truth():
    return gt_set(1, 3, [ann(0, 0, [0, 0, 10, 10])]), [det(0, 0, [0, 0, 10, 10], .9), det(0, 1, [0, 0, 10, 10], .8)], None


def ground_truth_without_detections():
    return gt_set(2, 2, [ann(0, 0, [0, 0, 10, 10]), ann(1, 1, [0, 0, 10, 10])]), [det(0, 0, [0, 0, 10, 10], .9)], None


def recall_stops_short():
    return (gt_set(1, 1, [ann(0, 0, [100 * n, 0, 20, 20]) for n in range(4)]),
            [det(0, 0, [0, 0, 20, 20], .9), det(0, 0, [300, 300, 20, 20], .8), det(0, 0, [100, 0, 20, 20], .7)], None)


def score_ties_across_images():
    # every score is .5: image 0 holds the false positive, images 1 and 2 the true positives
    return (gt_set(3, 1, [ann(1, 0, [0, 0, 10, 10]), ann(2, 0, [0, 0, 10, 10]), ann(0, 0, [0, 0, 10, 10])]),
            [det(2, 0, [0, 0, 10, 10], .5), det(1, 0, [0, 0, 10, 10], .5), det(0, 0, [100, 100, 10, 10], .5), det(0, 0, [0, 0, 10, 10], .25)], None)


def _many(n):
    anns = [ann(0, 0, [12 * (j % 32), 12 * (j // 32), 10, 10]) for j in range(n)]
    dts = [det(0, 0, [12 * 31, 12 * ((n - 1) // 32), 10, 10], .9), det(0, 0, [12 * ((n - 2) % 32), 12 * ((n - 2) // 32), 10, 8], .8),
           det(0, 0, [0, 0, 10, 10], .7), det(0, 0, [1000, 1000, 10, 10], .6)]
    return gt_set(1, 1, anns), dts, None


def ground_truths_1024():
    return _many(1024)


def ground_truths_1025():
    return _many(1025)


CASES = {f.__name__: f for f in (threshold_hit_exactly, threshold_above_the_cap, equal_iou_later_wins, crowd_matched_by_several,
                                 non_ignored_match_stops_the_walk, ignored_match_stays, ground_truth_outside_each_range,
                                 unmatched_detection_outside_the_range, boxes_that_only_touch, zero_area_boxes,
                                 more_detections_than_max_dets, one_sided_groups, category_without_ground_truth,
                                 ground_truth_without_detections, recall_stops_short, score_ties_across_images, ground_truths_1024)}


def mixed_set(seed=5, n_images=12, n_cats=5, n_gt=80, n_dt=300):
    """A seeded set with crowds, duplicate scores, detections of unknown images and categories, empty groups."""
    rng = np.random.default_rng(seed)
    anns = []
    for _ in range(n_gt):
        w, h = (rng.integers(8, 480, size=2) / 4)
        x, y = rng.integers(0, 1600) / 4, rng.integers(0, 1200) / 4
        anns.append(ann(int(rng.integers(n_images)), int(rng.integers(n_cats - 1)), [x, y, w, h], area=float(w * h * rng.choice([1.0, 0.75])),
                        crowd=int(rng.random() < 0.12)))
    dts = []
    for _ in range(n_dt):
        score = float(rng.integers(1, 40)) / 40
        if rng.random() < 0.7:
            a = anns[int(rng.integers(n_gt))]
            jitter = rng.integers(-8, 9, size=4) / 4
            b = [a['bbox'][0] + jitter[0], a['bbox'][1] + jitter[1], max(a['bbox'][2] + jitter[2], .25), max(a['bbox'][3] + jitter[3], .25)]
            img, cat = a['image_id'] // 10 - 1, a['category_id'] - 1
        else:
            b = [rng.integers(0, 1600) / 4, rng.integers(0, 1200) / 4, rng.integers(8, 480) / 4, rng.integers(8, 480) / 4]
            img, cat = int(rng.integers(n_images + 1)), int(rng.integers(n_cats + 1))            # one unknown image, one unknown category
        dts.append(det(img, cat, b, score))
    return gt_set(n_images, n_cats, anns), dts, None


# the seed of the rotated set: its reference IoUs all lie further than 9e-4 from every default threshold (tests/test_gpu_eval.py asserts 1e-4)
ROTATED_SEED = 8


def rotated_set(seed=ROTATED_SEED, n_images=4, n_gt=24, n_dt=70):
    """A seeded CEPDOF-like set: one category (detections carry no category_id), boxes (cx, cy, w, h, degrees), no area keys."""
    rng = np.random.default_rng(seed)
    anns = []
    for _ in range(n_gt):
        box = [float(rng.uniform(100, 900)), float(rng.uniform(100, 900)), float(rng.uniform(30, 160)), float(rng.uniform(30, 160)),
               float(rng.uniform(-90, 90))]
        a = {'image_id': 10 * (int(rng.integers(n_images)) + 1), 'category_id': 1, 'bbox': box}
        if len(anns) % 7 == 3:
            a['ignore'] = True
        anns.append(a)
    dts = []
    for _ in range(n_dt):
        if rng.random() < 0.75:
            a = anns[int(rng.integers(n_gt))]
            box = [a['bbox'][0] + float(rng.normal(0, 6)), a['bbox'][1] + float(rng.normal(0, 6)), a['bbox'][2] * float(rng.uniform(.8, 1.2)),
                   a['bbox'][3] * float(rng.uniform(.8, 1.2)), a['bbox'][4] + float(rng.normal(0, 8))]
            img = a['image_id']
        else:
            box = [float(rng.uniform(100, 900)), float(rng.uniform(100, 900)), float(rng.uniform(30, 160)), float(rng.uniform(30, 160)),
                   float(rng.uniform(-90, 90))]
            img = 10 * (int(rng.integers(n_images)) + 1)
        dts.append({'image_id': img, 'bbox': box, 'score': float(rng.integers(1, 50)) / 50})
    gt = {'images': [{'id': 10 * (i + 1), 'height': 1024, 'width': 1024} for i in range(n_images)], 'categories': [{'id': 1}], 'annotations': anns}
    return gt, dts, None
