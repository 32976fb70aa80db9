"""Box ops named by the hot path (reference: utils/bbox_ops.py:6-49, 309-316), and the rotated-box IoU / NMS of
utils/bbox_ops.py:52-100, 250-306 on the exact intersection area (iou_rotated, iou_rle, nms_rotbb)."""
import torch

from .. import ops


def bboxes_iou(bboxes_a, bboxes_b, xyxy=False):
    """Pairwise IoU [N,K] on the GPU, same arithmetic as the reference (chainercv form:
    intersection zeroed unless tl < br on both axes; no clamp, no epsilon)."""
    if bboxes_a.dim() == 1:
        bboxes_a = bboxes_a.unsqueeze(0)
    assert bboxes_a.dim() == bboxes_b.dim() == 2
    if bboxes_a.shape[1] != 4 or bboxes_b.shape[1] != 4:
        raise IndexError()
    if not bboxes_a.is_cuda:
        if not torch.cuda.is_available():
            raise RuntimeError('bboxes_iou runs on MI355X only; no GPU is visible')
        bboxes_a, bboxes_b = bboxes_a.cuda(), bboxes_b.cuda()
    return ops.bboxes_iou(bboxes_a, bboxes_b.to(bboxes_a.device), xyxy=xyxy)


def cxcywh_to_x1y1x2y2(cxcywh):
    """Centre-format boxes [..., >= 4] -> corner format, a new tensor (reference: utils/bbox_ops.py:309-316).  One
    launch of the to-corners kernel of csrc/boxops.hip: float32 `c - s / 2`, `c + s / 2` in the reference's operation
    order, so the result is bit-identical; extra columns (a rotated box's angle) are carried over."""
    assert cxcywh.shape[-1] >= 4
    # the reference returns a tensor of the input's device and dtype for any dtype: the kernel computes in float32
    # on the GPU; the result goes back to where and what the input was (float64 / integer inputs through a float32 round trip)
    src_device, src_dtype = cxcywh.device, cxcywh.dtype
    if not cxcywh.is_cuda:
        if not torch.cuda.is_available():
            raise RuntimeError('cxcywh_to_x1y1x2y2 runs on MI355X only; no GPU is visible')
        cxcywh = cxcywh.cuda()
    out = ops.cxcywh_to_x1y1x2y2(cxcywh if src_dtype == torch.float32 else cxcywh.float())
    return out.to(device=src_device, dtype=src_dtype)


def _on_gpu(t, what):
    if not t.is_cuda:
        if not torch.cuda.is_available():
            raise RuntimeError(f'{what} runs on MI355X only; no GPU is visible')
        t = t.cuda()
    return t


def iou_rotated(boxes1, boxes2, bb_format='cxcywhd'):
    """Pairwise IoU [N, M] float32 of rotated boxes, rows (cx, cy, w, h, degrees clockwise), on the device that holds
    boxes1 (moved to the GPU when on the host): the exact area of intersection of the two rectangles over their union, one
    launch of the pairwise kernel of csrc/boxops.hip.  The rectangles have the corners of the reference's xywha2vertex
    (utils/bbox_ops.py:137-172)."""
    if bb_format != 'cxcywhd':
        raise NotImplementedError()
    if boxes1.dim() != 2 or boxes2.dim() != 2 or boxes1.shape[1] != 5 or boxes2.shape[1] != 5:
        raise ValueError(f'iou_rotated: [N,5] and [M,5] boxes expected, got {tuple(boxes1.shape)} and {tuple(boxes2.shape)}')
    boxes1 = _on_gpu(boxes1, 'iou_rotated')
    return ops.rotated_iou(boxes1.float(), boxes2.to(boxes1.device).float())


def iou_rle(boxes1, boxes2, bb_format='cxcywhd', **kwargs):
    """IoU between rotated bounding boxes, under the reference's name and signature (utils/bbox_ops.py:52-100): tensors or
    numpy arrays of rows (cx, cy, w, h, degrees clockwise), 1-d inputs are one box; returns [N, M] float32 on the input's
    device (a numpy array with return_numpy=True).

    Deviation from the reference: it rasterises both boxes on an `img_hw` grid with pycocotools and counts pixels; this
    computes the EXACT area of intersection of the two rectangles (`iou_rotated`), so `img_hw` / `img_size` are accepted
    and ignored.  On tests/golden/rot_iou.npz the two differ by at most the discretisation error of the reference's own
    512^2 masks (rotated boxes)."""
    assert type(boxes1) == type(boxes2)
    assert bb_format == 'cxcywhd'
    if not (torch.is_tensor(boxes1) and torch.is_tensor(boxes2)):
        boxes1 = torch.from_numpy(boxes1).float()
        boxes2 = torch.from_numpy(boxes2).float()
    assert boxes1.device == boxes2.device
    device = boxes1.device
    if boxes1.dim() == 1:
        boxes1 = boxes1.unsqueeze(0)
    if boxes2.dim() == 1:
        boxes2 = boxes2.unsqueeze(0)
    assert boxes1.shape[1] == boxes2.shape[1] == 5
    ious = iou_rotated(boxes1, boxes2).to(device)
    if kwargs.get('return_numpy', False):
        return ious.cpu().numpy()
    return ious


def nms_rotbb(boxes, scores, nms_thres=0.45, bb_format='cxcywhd', img_size=2048, majority=None):
    """Single-class NMS for rotated boxes, under the reference's name and signature (utils/bbox_ops.py:250-306): greedy in
    score order, a box is dropped when its IoU with a kept box is >= nms_thres.  Returns the kept indices, int64, in score
    order (ties: lowest index first), on the device of `boxes`.  One launch of the post-process kernel with one class.
    The IoU is the exact intersection area (see `iou_rle`), so `img_size` is ignored.  At most 512 boxes, as in
    ImageObjects.non_max_suppression; majority voting is not provided."""
    if bb_format != 'cxcywhd':
        raise NotImplementedError()
    if majority is not None:
        raise NotImplementedError('nms_rotbb: majority voting is not provided')
    assert boxes.dim() == 2 and boxes.shape[1] == 5
    device = boxes.device
    n = boxes.shape[0]
    if n == 0:
        return torch.zeros(0, dtype=torch.int64, device=device)
    if n > ops.TOPK:
        raise NotImplementedError(f'nms_rotbb handles at most {ops.TOPK} boxes')
    bb = _on_gpu(boxes, 'nms_rotbb').float()
    sc = scores.to(bb.device).float().reshape(n)
    cats = torch.zeros(n, dtype=torch.int64, device=bb.device)
    rec = ops.postprocess(bb[None], cats[None], sc[None], float('-inf'), nms_thres, ops.TOPK, rotated_nms=True)
    k = ops.check_counts([int(rec['count'][0])])[0]
    return rec['index'][0, :k].to(device=device, dtype=torch.int64)
