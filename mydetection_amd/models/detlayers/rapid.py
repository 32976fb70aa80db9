"""RAPiD rotated-box decode layer (reference: models/detlayers/rapid.py)."""
import torch
import torch.nn as nn

from ... import ops
from ._common import alloc_outputs, pack_pixel_major


class RAPiDLayer(nn.Module):
    '''
    Inference branch of the reference RAPiDLayer (models/detlayers/rapid.py:11-81) as one fused HIP kernel
    (ops.DECODE_RAPID): cx=(sigmoid(tx)+x)*stride, cy likewise, w=exp(tw)*anchor_w, h likewise,
    deg=((sigmoid(ta)*2*pi - pi)/pi)*180; score=sigmoid(conf) without classes, sqrt(sigmoid(conf)*max_c sigmoid(cls_c))
    with them (class_idx = first argmax); flatten order (a,y,x).  Boxes are [B, N, 5] rows (cx, cy, w, h, deg), and the
    outputs stay in HBM.  Training (labels is not None) is out of scope.
    '''
    def __init__(self, level_i: int, cfg: dict):
        super().__init__()
        anchors_all = torch.Tensor(cfg['model.rapid.anchors'])
        indices = torch.Tensor(cfg['model.rapid.anchor_indices'][level_i]).long()
        self.anchor_indices = indices
        self.anchors = anchors_all[indices, :]
        self.anch_00wha_all = torch.zeros(len(anchors_all), 5)
        self.anch_00wha_all[:, 2:4] = anchors_all
        self.num_anchors = len(indices)
        self.stride = cfg['model.fpn.out_strides'][level_i]
        self.n_cls = cfg['general.num_class']
        self.ignore_thre = 0.6
        assert cfg.get('model.angle.pred_range', 360) == 360
        self.wh_sl1_beta = cfg.get('model.rapid.wh_smooth_l1_beta')

    def _layout(self, raw):
        """(box, ldbox, box_astride, box_c0, cls, ldcls, cls_astride, cls_c0, conf_c0) of the pixel-major head rows."""
        packed = getattr(raw, 'packed', None)
        if packed is not None:          # the head's own pixel-major tensors (YOLOHead: one; EfDetHead: box + class)
            return packed['box'] + packed['cls']
        parts = [raw['bbox'], raw['conf']] + ([raw['class']] if self.n_cls > 0 else [])
        box, ldb, per = pack_pixel_major(parts, self.num_anchors)
        return box, ldb, per, 0, box, ldb, per, 6, 5

    def forward(self, raw: dict, img_size, labels=None, _out=None):
        assert isinstance(raw, dict)
        if labels is not None:
            raise NotImplementedError('training/target assignment is outside the inference hot path')
        t_xywha = raw['bbox']
        nB, nA = t_xywha.shape[0], self.num_anchors
        nH, nW = t_xywha.shape[2:4]
        assert t_xywha.shape[1] == nA and t_xywha.shape[-1] == 5
        box, ldb, bas, bc0, cls, ldc, cas, cc0, conf0 = self._layout(raw)
        n = nA * nH * nW
        if _out is None:
            bbox, cls_idx, score = alloc_outputs(nB, n, box.device, box_width=5)
            n_off = 0
        else:
            bbox, cls_idx, score, n_off = _out
        ops.decode(ops.DECODE_RAPID, box, ldb, bas, bc0, cls, ldc, cas, cc0, conf0, self.anchors.numpy(), nA, self.n_cls,
                   nB, nH, nW, self.stride, tuple(img_size), bbox, cls_idx, score, n_off)
        preds = {
            'bbox': bbox[:, n_off:n_off + n],
            'class_idx': cls_idx[:, n_off:n_off + n],
            'score': score[:, n_off:n_off + n],
        }
        return preds, None

    def _describe(self, raw, img_size):
        """Level descriptor for the single-launch decode (ops.decode_levels), or None."""
        packed = getattr(raw, 'packed', None)
        if packed is None:
            return None
        box, ldb, bas, bc0 = packed['box']
        cls, ldc, cas, cc0, conf0 = packed['cls']
        nH, nW = raw['bbox'].shape[2:4]
        return {'mode': ops.DECODE_RAPID, 'layout': (bas, bc0, cas, cc0, conf0), 'A': self.num_anchors, 'C': self.n_cls,
                'level': {'box': box, 'ldbox': ldb, 'cls': cls, 'ldcls': ldc, 'anchors_wh': self.anchors.numpy(),
                          'H': nH, 'W': nW, 'stride': self.stride}}
