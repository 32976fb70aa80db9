"""Drawing detections on images (reference: utils/visualization.py:77-137, draw_bboxes_on_np).  The reference draws with cv2 on
the host; here the image makes one trip to the device and the overlay renderer paints it (ops.draw_boxes; include/mydet.h has
the raster rules).  Call shape and intent are the reference's, the pixels are this package's."""
import numpy as np
import torch

from .. import ops

CLASS_MAPS = ('COCO', 'ImageNet')        # accepted as in the reference; the package ships no name table (class_names= gives one)


def objects_to_rows(objs_list, device):
    """Dense device rows of a list of ImageObjects for ops.draw_boxes: (boxes [B,K,4|5], counts int32 [B], scores [B,K] or
    None, classes int64 [B,K], ids int64 [B,K] or None), K the largest count (zero rows pad the others)."""
    B = len(objs_list)
    K = max([len(o) for o in objs_list] + [1])
    width = max([o.bboxes.shape[1] for o in objs_list if len(o)] + [4])
    boxes = torch.zeros((B, K, width), dtype=torch.float32, device=device)
    classes = torch.zeros((B, K), dtype=torch.int64, device=device)
    has_scores = all(o.scores is not None for o in objs_list)
    has_ids = all(getattr(o, 'obj_ids', None) is not None for o in objs_list)
    scores = torch.zeros((B, K), dtype=torch.float32, device=device) if has_scores else None
    ids = torch.zeros((B, K), dtype=torch.int64, device=device) if has_ids else None
    for b, o in enumerate(objs_list):
        n = len(o)
        if n == 0:
            continue
        boxes[b, :n] = o.bboxes.to(device=device, dtype=torch.float32)
        classes[b, :n] = o.cats.to(device)
        if has_scores:
            scores[b, :n] = o.scores.to(device=device, dtype=torch.float32)
        if has_ids:
            ids[b, :n] = o.obj_ids.to(device)
    counts = torch.tensor([len(o) for o in objs_list], dtype=torch.int32).to(device)
    return boxes, counts, scores, classes, ids


def draw_bboxes_on_np(im, img_objs, class_map='COCO', **kwargs):
    '''
    Draw bounding boxes on a numpy image in-place (one copy to the device, one launch, one copy back).

    Args:
        im: numpy.ndarray, uint8, shape(h,w,3), RGB
        img_objs: utils.structures.ImageObjects ('cxcywh' or 'cxcywhd'); obj_ids, when present, add '#id' to the label and
                  select the colour
        class_map: 'COCO' or 'ImageNet' are accepted; no name table ships with the package, so without class_names the
                   label shows the class index
        color: (r, g, b) for every box (default: by class, or by id with obj_ids); line_width (default max(1, round(h / 360)));
        put_text (default True); show_class (default True); class_names: list of str; label_height; fill_alpha
    '''
    if not isinstance(im, np.ndarray) or im.dtype != np.uint8 or im.ndim != 3 or im.shape[2] != 3:
        raise TypeError('draw_bboxes_on_np: im is a numpy uint8 array of shape (h, w, 3)')
    if class_map not in CLASS_MAPS:
        raise NotImplementedError()
    if img_objs._bb_format not in ('cxcywh', 'cxcywhd'):
        raise NotImplementedError()
    h = im.shape[0]
    has_ids = getattr(img_objs, 'obj_ids', None) is not None
    labels = []
    if kwargs.get('put_text', True):
        labels = (['class'] if kwargs.get('show_class', True) else []) + (['score'] if img_objs.scores is not None else []) + \
                 (['id'] if has_ids else [])
    color = kwargs.get('color', None)
    style = ops.draw_style(thickness=int(kwargs.get('line_width', max(1, round(h / 360)))), fill_alpha=int(kwargs.get('fill_alpha', 0)),
                           color_by='id' if has_ids else 'class', color=color, labels=labels,
                           label_height=int(kwargs.get('label_height', default_label_height(h))), class_names=kwargs.get('class_names'))
    if len(img_objs) == 0:
        return im
    if not torch.cuda.is_available():
        raise RuntimeError('draw_bboxes_on_np: the renderer is a HIP kernel; no GPU is visible')
    dev = torch.device('cuda')
    frame = torch.from_numpy(np.ascontiguousarray(im)).to(dev)
    boxes, counts, scores, classes, ids = objects_to_rows([img_objs], dev)
    ops.draw_boxes(frame, boxes, style, counts=counts, scores=scores, classes=classes, ids=ids)
    im[...] = frame.cpu().numpy()
    return im


def default_label_height(h):
    """Rows of a label cell for a frame of h rows when none is asked for: round(h / 45) kept inside 10..64 (24 at 1080)."""
    return int(min(64, max(10, round(h / 45))))
