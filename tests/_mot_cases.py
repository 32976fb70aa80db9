"""Ground truths and hypothesis rows for the track-scorer tests, hand-written or generated from a fixed seed (test code).

A scene is a list of sequences; a sequence is a list of frames; a frame is (ground truths, hypotheses), each a list of
(identity, box[, category]).  `build` turns it into the ground-truth dict (images with video_id / frame_id, annotations with
track_id) and the hypothesis rows.
"""
import numpy as np


def build(scene, n_cats=1, id_key='track_id', video_ids=True):
    images, anns, rows = [], [], []
    for s, frames in enumerate(scene):
        for f, (gts, hyps) in enumerate(frames):
            img = 1000 * (s + 1) + f
            im = {'id': img, 'file_name': f'{s}_{f}.jpg'}
            if video_ids:
                im.update(video_id=s, frame_id=f)
            images.append(im)
            for item in gts:
                box = [float(v) for v in item[1]]
                anns.append({'id': len(anns) + 1, 'image_id': img, 'category_id': item[2] if len(item) > 2 else 1, 'bbox': box,
                             'area': box[2] * box[3], 'iscrowd': 0, id_key: item[0]})
            for item in hyps:
                rows.append({'image_id': img, 'category_id': item[2] if len(item) > 2 else 1, 'bbox': [float(v) for v in item[1]],
                             'score': 1.0, 'track_id': item[0]})
    gt = {'images': images, 'categories': [{'id': k + 1, 'name': f'c{k + 1}'} for k in range(n_cats)], 'annotations': anns}
    return gt, rows


def box(x, y=0.0, w=10.0, h=10.0):
    return [x, y, w, h]


def shifted(iou):
    """A 10 x 10 box at x such that its IoU with box(0) is about `iou`: (10 - x) / (10 + x)."""
    return box(10.0 * (1 - iou) / (1 + iou))


def swap():
    """Sequence 0: two objects cross and the hypotheses exchange identities (2 switches).  Sequence 1: no exchange."""
    a, b = box(0), box(100)
    crossing = [([(1, a), (2, b)], [(7, a), (8, b)]), ([(1, a), (2, b)], [(7, a), (8, b)]),
                ([(1, a), (2, b)], [(8, a), (7, b)]), ([(1, a), (2, b)], [(8, a), (7, b)])]
    steady = [([(1, a), (2, b)], [(7, a), (8, b)])] * 4
    return [crossing, steady]


def keep_beats_cheaper():
    """Frame 1 alone would pair gt 1 with hyp 8 (IoU 1.0) and gt 2 with hyp 7; the previous correspondence 1-7 (IoU ~0.6) and
    2-8 is still eligible at 0.5 and is kept."""
    first = ([(1, box(0)), (2, box(100))], [(7, box(0)), (8, box(100))])
    near = box(2.5)                                                   # IoU with box(0): 7.5 / 12.5 = 0.6
    second = ([(1, box(0)), (2, near)], [(7, near), (8, box(0))])
    return [[first, second]]


def shared_last():
    """Ground truths 1 and 2 both have last = 7: 1 was matched to 7 in frame 0, 2 in frame 1 (where 1 is absent).  In frame 2 both
    overlap hypothesis 7; the lower row wins and row 1 (gt 2) goes to the assignment."""
    return [[([(1, box(0))], [(7, box(0))]),
             ([(2, box(1))], [(7, box(1))]),
             ([(1, box(0)), (2, box(1))], [(7, box(1)), (9, box(0.5))])]]


def greedy_loses():
    """One frame of two ground truths and two hypotheses; the test supplies the IoUs [[0.9, 0.6], [0.55, 0.1]] (rows ground truths)
    as GREEDY_IOUS, the buffer in its hypothesis-major layout.  At threshold 0.5: row0 -> col1, row1 -> col0."""
    return [[([(1, box(0)), (2, box(3))], [(7, box(1)), (8, box(2))])]]


GREEDY_IOUS = [0.9, 0.55, 0.6, 0.1]


def persistent_last():
    """Object 1 is matched to 7, unmatched for two frames, then matched to 9: one switch and one fragmentation."""
    a, far = box(0), box(500)
    return [[([(1, a)], [(7, a)]), ([(1, a)], [(7, far)]), ([(1, a)], []), ([(1, a)], [(9, a)])]]


def sizes(n_rows, n_cols, seed):
    """One sequence: a frame of n_rows ground truths against n_cols jittered hypotheses, then the empty kinds of frame (no ground
    truth, no hypotheses, neither), then the first frame again with the hypotheses in another order."""
    rng = np.random.default_rng(seed)
    side = int(np.ceil(np.sqrt(max(n_rows, n_cols))))
    cells = rng.permutation(side * side)
    gts = [(i, [30.0 * (c % side) + rng.uniform(-4, 4), 30.0 * (c // side) + rng.uniform(-4, 4), 20.0, 20.0]) for i, c in enumerate(cells[:n_rows])]
    cells = rng.permutation(side * side)
    hyps = [(1000 + i, [30.0 * (c % side) + rng.uniform(-6, 6), 30.0 * (c // side) + rng.uniform(-6, 6), rng.uniform(16, 24), rng.uniform(16, 24)])
            for i, c in enumerate(cells[:n_cols])]
    again = [hyps[i] for i in rng.permutation(len(hyps))]
    return [[(gts, hyps), ([], hyps[:3]), (gts[:3], []), ([], []), (gts, again)]]


def several(seed=5, S=3, K=2, frames=6, n=7):
    """S sequences x K categories of a few drifting objects with dropped, spurious and relabelled hypotheses."""
    rng = np.random.default_rng(seed)
    scene = []
    for s in range(S):
        pos = rng.uniform(0, 300, (n, 2))
        cat = rng.integers(1, K + 1, n)
        label = np.arange(n) + 50
        seq = []
        for f in range(frames + s):
            pos = pos + rng.uniform(-3, 3, (n, 2))
            if f == 3:
                label[:2] = label[:2][::-1] + 0
            gts = [(i, [pos[i, 0], pos[i, 1], 24.0, 24.0], int(cat[i])) for i in range(n) if rng.random() > 0.15]
            hyps = [(int(label[i]), [pos[i, 0] + rng.uniform(-5, 5), pos[i, 1] + rng.uniform(-5, 5), 24.0, 24.0], int(cat[i])) for i in range(n)
                    if rng.random() > 0.2]
            hyps += [(900 + f, [rng.uniform(0, 300), rng.uniform(0, 300), 24.0, 24.0], int(rng.integers(1, K + 1)))]
            seq.append((gts, hyps))
        scene.append(seq)
    return scene


def id_case():
    """Hypothesis 7 covers ground truth 1 for three frames and ground truth 2 for four; hypothesis 8 covers ground truth 1 for the
    last four.  Per frame everything matches (TP = 7 + ...), but one-to-one over the sequence 7 can only stand for one of them."""
    a, b = box(0), box(100)
    frames = [([(1, a)], [(7, a)])] * 3 + [([(1, a), (2, b)], [(8, a), (7, b)])] * 4
    return [frames]


def id_random(n_g=70, n_h=90, frames=12, seed=3):
    """n_g ground-truth identities on a grid; n_h hypothesis identities that hop between them every few frames."""
    rng = np.random.default_rng(seed)
    side = int(np.ceil(np.sqrt(n_g)))
    cell = [[40.0 * (i % side), 40.0 * (i // side), 20.0, 20.0] for i in range(n_g)]
    seq = []
    owner = rng.permutation(n_h)
    for f in range(frames):
        if f % 3 == 0:
            owner = rng.permutation(n_h)
        gts = [(i, cell[i]) for i in range(n_g) if rng.random() > 0.1]
        hyps = []
        for h in range(n_h):
            i = int(owner[h])
            if i < n_g and rng.random() > 0.1:
                hyps.append((h, [cell[i][0] + rng.uniform(-3, 3), cell[i][1] + rng.uniform(-3, 3), 20.0, 20.0]))
            elif i >= n_g:
                hyps.append((h, [rng.uniform(0, 300), 2000.0 + 40.0 * h, 20.0, 20.0]))
        seq.append((gts, hyps))
    return [seq]
