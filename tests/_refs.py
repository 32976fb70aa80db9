"""float64 restatements shared by the footprint and branch-coverage tests (plain torch, CPU)."""
import torch
import torch.nn.functional as F


def act_f64(y, act):
    """The conv epilogue's activation codes: 0 none, 1 LeakyReLU(0.1), 2 swish."""
    if act == 1:
        return F.leaky_relu(y, 0.1)
    if act == 2:
        return y * torch.sigmoid(y)
    return y


def sepconv_node_f64(inputs, modes, fuse_w, w_dw, w_pw, scale, shift, act):
    """One pyramid node: [fusion + swish ->] depthwise 3x3 -> pointwise (+ folded BN, act).  modes: 0 same size, 1 half-size map
    through nearest 2x, 2 double-size map through max_pool2d(3, 2, 1)."""
    ins = []
    for t, m in zip(inputs, modes):
        t = t.double()
        if m == 1:
            t = F.interpolate(t, scale_factor=(2, 2), mode='nearest')
        elif m == 2:
            t = F.max_pool2d(t, 3, 2, 1)
        ins.append(t)
    if len(ins) > 1:
        w = F.relu(fuse_w.double())
        w = w / (w.sum() + 0.0001)
        x = sum(wi * f for wi, f in zip(w, ins))
        x = x * torch.sigmoid(x)
    else:
        x = ins[0]
    C = x.shape[1]
    y = F.conv2d(x, w_dw.double().permute(2, 0, 1).reshape(C, 1, 3, 3), None, 1, 1, 1, C)
    y = F.conv2d(y, w_pw.double().reshape(w_pw.shape[0], C, 1, 1))
    y = y * (scale.double().view(1, -1, 1, 1) if scale is not None else 1.0) + shift.double().view(1, -1, 1, 1)
    return act_f64(y, act)


def retina_decode_f64(cls_logits, box_logits, anchors_wh, stride, img_hw):
    """RetinaLayer (models/detlayers/retinanet.py) on float64 head logits [B, A*n_cls, H, W] / [B, A*4, H, W], candidates in
    (a, y, x) order: centre = stride/2 + x*stride + t*aw, size = exp(t)*aw, all four clamped to [1, max(img_h, img_w)];
    score = sigmoid(max logit), class = argmax.  Returns bbox [B,N,4], raw (bbox before the clamp), anchor ([B,N,4]: aw, ah, aw, ah),
    score, class_idx [B,N] and gap [B,N], the distance between the two largest logits of a candidate."""
    B, _, H, W = box_logits.shape
    A = anchors_wh.shape[0]
    cl = cls_logits.double().view(B, A, -1, H, W)
    top = cl.topk(2, dim=2)
    t = box_logits.double().view(B, A, 4, H, W)
    aw, ah = (anchors_wh.double()[:, i].view(1, A, 1, 1) for i in (0, 1))
    acx = (stride / 2 + torch.arange(W, dtype=torch.float64) * stride).view(1, 1, 1, W)
    acy = (stride / 2 + torch.arange(H, dtype=torch.float64) * stride).view(1, 1, H, 1)
    raw = torch.stack([acx + t[:, :, 0] * aw, acy + t[:, :, 1] * ah, torch.exp(t[:, :, 2]) * aw, torch.exp(t[:, :, 3]) * ah], dim=-1)
    anchor = torch.stack([aw, ah, aw, ah], dim=-1).expand(B, A, H, W, 4)
    return dict(bbox=raw.clamp(1.0, float(max(img_hw))).reshape(B, -1, 4), raw=raw.reshape(B, -1, 4), anchor=anchor.reshape(B, -1, 4),
                score=torch.sigmoid(top.values[:, :, 0]).reshape(B, -1), class_idx=top.indices[:, :, 0].reshape(B, -1),
                gap=(top.values[:, :, 0] - top.values[:, :, 1]).reshape(B, -1))


def lr_tb_layer_f64(x, lr0, tb0, lr1, blr, tb1, btb):
    """The lr_tb box layer: two depthwise 3x3 convs, a (1,3) conv for (l, r) and a (3,1) conv for (t, b) on their zero-padded
    outputs; x [B,C,H,W] -> [B,4,H,W] in (l, t, r, b) order."""
    x = x.double()
    C = x.shape[1]
    dlr = F.conv2d(x, lr0.double(), None, 1, 1, 1, C)
    dtb = F.conv2d(x, tb0.double(), None, 1, 1, 1, C)
    lr = F.conv2d(dlr, lr1.double(), blr.double(), 1, (0, 1))
    tb = F.conv2d(dtb, tb1.double(), btb.double(), 1, (1, 0))
    return torch.stack([lr[:, 0], tb[:, 0], lr[:, 1], tb[:, 1]], dim=1)


def se_gate_f64(y, w1, b1, w2t, b2):
    """Squeeze-excite gate of a map y [B,C,H,W]: sigmoid(W2 . swish(W1 . mean_pixels(y) + b1) + b2); w2t = W2 transposed [Cse,C]."""
    m = y.double().mean(dim=(2, 3))
    h = m @ w1.double().t() + b1.double()
    h = h * torch.sigmoid(h)
    return torch.sigmoid(h @ w2t.double() + b2.double())
