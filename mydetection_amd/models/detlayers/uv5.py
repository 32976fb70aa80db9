"""Ultralytics (YOLOv5) decode layer (reference: models/detlayers/uv5.py)."""
import torch
import torch.nn as nn

from ... import ops
from ._common import alloc_outputs, pack_pixel_major


class DetectLayer(nn.Module):
    '''
    Inference branch of the reference DetectLayer (models/detlayers/uv5.py:42-91) as one fused HIP kernel
    (ops.decode_uv5_levels): s=sigmoid(t[0..3]), cx=(s0*2-0.5+x)*stride, cy likewise, w=(s2*2)**2*anchor_w, h likewise,
    score=sigmoid(conf)*max_c sigmoid(cls_c), class_idx=first argmax; flatten order (a,y,x).  Centres reach down to
    -stride/2 and w, h up to 4*anchor; nothing is clamped.  The outputs stay in HBM.
    Training (labels is not None) and 'cxcywhd' boxes are out of scope.
    '''
    def __init__(self, level_i: int, cfg: dict):
        super().__init__()
        anchors_all = torch.Tensor(cfg['model.detect.anchors'])
        indices = torch.Tensor(cfg['model.detect.anchor_indices'][level_i]).long()
        self.indices = indices
        self.anchors = anchors_all[indices, :]
        self.anch_00wh_all = torch.zeros(len(anchors_all), 4)
        self.anch_00wh_all[:, 2:4] = anchors_all
        self.num_anchors = len(indices)
        self.stride = cfg['model.fpn.out_strides'][level_i]
        self.strides_all = cfg['model.fpn.out_strides']
        self.n_cls = cfg['general.num_class']
        self.bbox_format = cfg['general.pred_bbox_format']
        # read by the training branch only
        self.sample_selection = cfg.get('model.detect.sample_selection')
        self.conf_target = cfg.get('model.detect.confidence_target')
        self.negative_thres = cfg.get('model.detect.negative_threshold', 0.7)
        self.loss_bbox = cfg.get('model.detect.loss_bbox')

    def _layout(self, raw):
        """(box, ldbox, box_astride, box_c0, cls, ldcls, cls_astride, cls_c0, conf_c0) of the pixel-major head rows."""
        packed = getattr(raw, 'packed', None)
        if packed is not None:          # the head's own pixel-major tensors (YOLOHead: one; EfDetHead: box + class)
            return packed['box'] + packed['cls']
        box, ldb, per = pack_pixel_major([raw['bbox'], raw['conf'], raw['class']], self.num_anchors)
        return box, ldb, per, 0, box, ldb, per, 5, 4

    def forward(self, raw: dict, img_size, labels=None, _out=None):
        assert isinstance(raw, dict)
        if labels is not None:
            raise NotImplementedError('training/target assignment is outside the inference hot path')
        if self.bbox_format != 'cxcywh':
            raise NotImplementedError()
        t_bbox = raw['bbox']
        nB, nA = t_bbox.shape[0], self.num_anchors
        nH, nW = t_bbox.shape[2:4]
        assert t_bbox.shape[1] == nA and t_bbox.shape[-1] == 4
        assert self.n_cls > 0
        box, ldb, bas, bc0, cls, ldc, cas, cc0, conf0 = self._layout(raw)
        n = nA * nH * nW
        if _out is None:
            bbox, cls_idx, score = alloc_outputs(nB, n, box.device)
            n_off = 0
        else:
            bbox, cls_idx, score, n_off = _out
        ops.decode_uv5(box, ldb, bas, bc0, cls, ldc, cas, cc0, conf0, self.anchors.numpy(), nA, self.n_cls, nB, nH, nW,
                       self.stride, tuple(img_size), bbox, cls_idx, score, n_off)
        preds = {
            'bbox': bbox[:, n_off:n_off + n],
            'class_idx': cls_idx[:, n_off:n_off + n],
            'score': score[:, n_off:n_off + n],
        }
        return preds, None

    def _describe(self, raw, img_size):
        """Level descriptor for the single-launch decode (ops.decode_uv5_levels, named by 'launch'), or None."""
        packed = getattr(raw, 'packed', None)
        if packed is None or self.bbox_format != 'cxcywh':
            return None
        box, ldb, bas, bc0 = packed['box']
        cls, ldc, cas, cc0, conf0 = packed['cls']
        nH, nW = raw['bbox'].shape[2:4]
        return {'mode': None, 'launch': ops.decode_uv5_levels, 'layout': (bas, bc0, cas, cc0, conf0),
                'A': self.num_anchors, 'C': self.n_cls,
                'level': {'box': box, 'ldbox': ldb, 'cls': cls, 'ldcls': ldc, 'anchors_wh': self.anchors.numpy(),
                          'H': nH, 'W': nW, 'stride': self.stride}}
