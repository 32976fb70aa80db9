"""Detection container + post-processing (reference: utils/structures.py:11-259).

Same fields and methods as the reference ``ImageObjects``; ``post_process`` / ``nms`` run the
batched HIP kernel (filter -> top-512 -> class-aware NMS) on the device that holds the
candidates instead of copying all N candidates to the host and looping over classes with
torchvision.ops.nms.  Results (order included) are those of the reference: class id
ascending, score descending inside a class.  Rotated boxes ('cxcywhd', rows (cx, cy, w, h, deg)) take the same kernel
on columns 0-3 -- the reference's NMS ignores the angle too (utils/structures.py:137-149) -- with the angle carried along.
`rotated_nms=True` / `rotated=True` (opt-in, 'cxcywhd' only) runs the NMS on the rotated rectangles instead: exact
intersection area, suppress at IoU >= nms_thres -- what the reference's commented-out nms_rotbb branch
(utils/structures.py:144-148) would do, with an exact area in place of its rasterised masks.
"""
import torch

from .. import ops

TOPK = 512          # utils/structures.py:99-101


class ImageObjects():
    '''
    A group of image bounding boxes

    Args:
        bboxes: 2-d tensor, torch.float32
        cats: 1-d tensor, torch.int64, categories
        scores (optional): 1-d tensor, torch.float32, scores
        bb_format (optional): 'cxcywh', or 'cxcywhd' (rotated boxes: cx, cy, w, h, angle in degrees)
        img_hw: tuple-like, image (height, width)
        obj_ids (optional): 1-d tensor, torch.int64, persistent track identities (Detector.predict_frames(tracker=)); else None
        zone_mask, line_events (optional): 1-d tensors, torch.int32, per object: the polygons it is inside (bit z) and the lines
            it went through in this frame (bit 2l positive, 2l+1 negative) (Detector.predict_frames(tracker=, zones=)); else None
    '''
    _PER_OBJECT = ('obj_ids', 'zone_mask', 'line_events')            # optional 1-d fields that follow every selection of rows

    def __init__(self, bboxes, cats, masks=None, scores=None, bb_format='cxcywh', img_hw=None, obj_ids=None, zone_mask=None,
                 line_events=None):
        self.obj_ids: torch.LongTensor = obj_ids
        self.zone_mask: torch.IntTensor = zone_mask
        self.line_events: torch.IntTensor = line_events
        self.bboxes: torch.FloatTensor = bboxes
        self.cats: torch.LongTensor = cats
        self.masks: torch.BoolTensor = masks
        self.scores: torch.FloatTensor = scores
        self._bb_format: str = bb_format
        self.img_hw: tuple = img_hw
        self.sanity_check()

    def __getitem__(self, idx):
        if isinstance(idx, int):
            idx = slice(idx, idx + 1)
        b = self.bboxes[idx, :]
        c = self.cats[idx]
        m = self.masks[idx, :, :] if self.masks is not None else None
        s = self.scores[idx] if self.scores is not None else None
        return ImageObjects(b, c, m, s, self._bb_format, self.img_hw, **self._per_object(lambda t: t[idx]))

    def _per_object(self, fn):
        """fn applied to each optional per-object field that is set, as keyword arguments of the constructor."""
        return {k: None if getattr(self, k) is None else fn(getattr(self, k)) for k in self._PER_OBJECT}

    def _per_object_(self, fn):
        for k, v in self._per_object(fn).items():
            setattr(self, k, v)

    def __len__(self):
        return self.bboxes.shape[0]

    def cpu_(self):
        '''Move all attributes to CPU in-place'''
        self.bboxes = self.bboxes.cpu()
        self.cats = self.cats.cpu()
        self.scores = self.scores.cpu() if self.scores is not None else None
        self.masks = self.masks.cpu() if self.masks is not None else None
        self._per_object_(lambda t: t.cpu())

    def cuda_(self, device='cuda'):
        '''Move all attributes to the GPU in-place (the kernels need them there)'''
        self.bboxes = self.bboxes.to(device)
        self.cats = self.cats.to(device)
        self.scores = self.scores.to(device) if self.scores is not None else None
        self.masks = self.masks.to(device) if self.masks is not None else None
        self._per_object_(lambda t: t.to(device))

    def sort_by_score_(self, descending=True):
        '''Sort the bounding boxes by scores in-place'''
        assert self.scores is not None
        assert self.masks is None, 'sorting with masks is not currently supported'
        idxs = torch.argsort(self.scores, descending=descending)
        self.bboxes = self.bboxes[idxs, :]
        self.cats = self.cats[idxs]
        self.scores = self.scores[idxs]
        self._per_object_(lambda t: t[idxs])

    def category_filter_(self, categories) -> None:
        '''Keep the objects in the given category set and discard others in-place.'''
        assert self.masks is None, 'filtering with masks is not currently supported'
        keep_cats = torch.as_tensor(list(categories), dtype=torch.int64, device=self.cats.device)
        assert self.cats.dim() == 1 and keep_cats.dim() == 1
        keep_mask = (self.cats.unsqueeze(1) == keep_cats.unsqueeze(0)).any(dim=1)
        self.bboxes = self.bboxes[keep_mask]
        self.cats = self.cats[keep_mask]
        if self.scores is not None:
            self.scores = self.scores[keep_mask]
        self._per_object_(lambda t: t[keep_mask])

    # ------------------------------------------------------------------ post-processing
    def _device_fields(self):
        if not self.bboxes.is_cuda:
            if not torch.cuda.is_available():
                raise RuntimeError('ImageObjects post-processing runs on MI355X only; no GPU is visible '
                                   '(mydetection_amd has no CPU path)')
            self.cuda_()
        return self.bboxes.contiguous(), self.cats.contiguous(), self.scores.contiguous()

    def _from_records(self, rec, b=0):
        k = ops.check_counts([int(rec['count'][b])])[0]          # the one host sync: how many survived
        return ImageObjects(ops.record_boxes(rec, b, k), rec['class_idx'][b, :k], None, rec['score'][b, :k],
                            self._bb_format, img_hw=self.img_hw)

    def post_process(self, conf_thres, nms_thres, rotated_nms=False, nms=None):
        '''
        Confidence threshold + top-512 + class-aware NMS (reference: utils/structures.py:92-106),
        one HIP launch.  Returns a new ImageObjects whose tensors stay on the device.
        rotated_nms: compare the rotated rectangles ('cxcywhd' only; ValueError otherwise).
        nms: None, or an ops.Nms (class-agnostic suppression, Soft-NMS, box merging; not with rotated_nms: ValueError).
        '''
        assert self.masks is None
        assert self.scores is not None
        _check_rotated(rotated_nms, self._bb_format)
        if self._bb_format not in _BOX_WIDTH:
            raise NotImplementedError()
        ops.nms_mode('post_process', nms, conf_thres, _BOX_WIDTH[self._bb_format], rotated_nms)     # the rules, before any device
        bb, cats, sc = self._device_fields()
        rec = ops.postprocess(bb[None], cats[None], sc[None], conf_thres, nms_thres, TOPK, rotated_nms=rotated_nms, nms=nms)
        return self._from_records(rec)

    def nms(self, nms_thres=0.45, rotated=False, nms=None):
        return ImageObjects.non_max_suppression(self, nms_thres, rotated=rotated, nms=nms)

    @staticmethod
    def non_max_suppression(dts, nms_thres: float, rotated=False, nms=None):
        '''
        Class-aware NMS (reference: utils/structures.py:111-173).  At most 512 boxes, as in the
        reference call chain (post_process caps at 512 before calling nms).
        rotated: compare the rotated rectangles ('cxcywhd' only; ValueError otherwise).
        nms: None, or an ops.Nms with agnostic alone (every box is a candidate here, whatever its score; the soft kinds and
        'merge' need a confidence threshold and raise ValueError: use post_process).
        '''
        assert isinstance(dts, ImageObjects)
        assert dts.masks is None, 'nms with masks is not currently supported'
        assert dts.scores is not None
        _check_rotated(rotated, dts._bb_format)
        if dts._bb_format in _BOX_WIDTH:
            ops.nms_mode('non_max_suppression', nms, float('-inf'), _BOX_WIDTH[dts._bb_format], rotated)
        if dts.bboxes.shape[0] == 0:
            return dts
        if dts._bb_format not in _BOX_WIDTH:
            raise NotImplementedError()
        if len(dts) > TOPK:
            raise NotImplementedError(f'non_max_suppression handles at most {TOPK} boxes per image')
        bb, cats, sc = dts._device_fields()
        rec = ops.postprocess(bb[None], cats[None], sc[None], float('-inf'), nms_thres, TOPK, rotated_nms=rotated, nms=nms)
        return dts._from_records(rec)

    def bboxes_to_original_(self, pad_info):
        '''
        Recover the bbox from the padded image to the original image
        (reference: utils/structures.py:175-189).  pad_info: (ori w, ori h, tl x, tl y, imw, imh).  Columns 0-3 only: the
        angle of a 'cxcywhd' box is unchanged.
        '''
        assert self.masks is None, 'this func with masks is not currently supported'
        assert len(pad_info) == 6
        ori_w, ori_h = pad_info[0], pad_info[1]
        if len(self) > 0:
            if not self.bboxes.is_cuda:
                self._device_fields()
            self.bboxes = self.bboxes.contiguous()
            if self.bboxes.shape[1] == 4:
                ops.bboxes_to_original_(self.bboxes, pad_info)
            else:
                xywh = self.bboxes[:, :4].contiguous()
                ops.bboxes_to_original_(xywh, pad_info)
                self.bboxes[:, :4] = xywh
        self.img_hw = (ori_h, ori_w)

    def draw_on_np(self, np_img, class_map='COCO', **kwargs):
        """Draw the boxes on a numpy uint8 image [h,w,3] in place (reference: utils/structures.py:215-219); see
        utils.visualization.draw_bboxes_on_np for the keywords."""
        from .visualization import draw_bboxes_on_np
        return draw_bboxes_on_np(np_img, self, class_map=class_map, **kwargs)

    def sanity_check(self):
        '''Integrity check (reference: utils/structures.py:191-213).'''
        assert self.bboxes.dtype == torch.float and self.bboxes.dim() == 2
        if self._bb_format == 'cxcywh':
            assert self.bboxes.shape[1] == 4
        elif self._bb_format == 'cxcywhd':
            assert self.bboxes.shape[1] == 5
        else:
            raise NotImplementedError()
        assert self.cats.dtype == torch.int64, 'Incorrect data type of categories'
        assert self.cats.dim() == 1 and self.cats.shape[0] == self.bboxes.shape[0]
        if self.masks is not None:
            assert self.masks.dtype == torch.bool and self.masks.dim() == 3
            assert self.masks.shape == (self.cats.shape[0],) + tuple(self.img_hw)
        if self.scores is not None:
            assert self.scores.shape[0] == self.bboxes.shape[0]
        assert self.img_hw is None or len(self.img_hw) == 2
        for k in ('zone_mask', 'line_events'):
            t = getattr(self, k)
            assert t is None or (t.dtype == torch.int32 and t.dim() == 1 and t.shape[0] == self.bboxes.shape[0]), k

    def to_json(self, img_id, eval_type='x1y1wh', catIdx2id=None) -> list:
        '''
        COCO-like json (reference: utils/structures.py:221-259).  The numbers (x1 = cx - w/2 ... in the reference's
        Python-float, i.e. double, arithmetic; category ids) come from one HIP launch and one device->host copy.
        '''
        assert self.bboxes.dim() == 2
        assert self.bboxes.shape[0] == self.cats.shape[0] == self.scores.shape[0]
        if eval_type == 'cxcywhd':
            assert self._bb_format == 'cxcywhd'
            return _json_rotated(self.bboxes.cpu(), self.scores.cpu(), self.cats.cpu(), img_id, catIdx2id)
        if eval_type != 'x1y1wh':
            raise NotImplementedError()
        assert self._bb_format == 'cxcywh'
        if len(self) == 0:
            return []
        bb, cats, sc = self._device_fields()
        table, host_map = _category_table(catIdx2id, bb.device)
        rows, cat = ops.detections_to_json(bb.contiguous()[None], sc.contiguous()[None], cats.contiguous()[None], None, table)
        return _json_rows(rows[0].cpu().tolist(), cat[0].cpu().tolist(), img_id, host_map)


_BOX_WIDTH = {'cxcywh': 4, 'cxcywhd': 5}


def _check_rotated(rotated_nms, bb_format):
    if rotated_nms and bb_format != 'cxcywhd':
        raise ValueError(f"rotated NMS is defined for bb_format 'cxcywhd' only, not {bb_format!r}")


def _json_rotated(bboxes, scores, cats, img_id, catIdx2id):
    """to_json(eval_type='cxcywhd') (reference: utils/structures.py:245-247): the five box values as Python floats, no
    arithmetic, so it runs on the host copy of the detections."""
    from .constants import COCO_CATEGORY_IDS
    table = COCO_CATEGORY_IDS if catIdx2id is None else catIdx2id
    return [{'image_id': img_id, 'category_id': table[int(c)], 'bbox': [float(t) for t in bb], 'score': float(s)}
            for bb, c, s in zip(bboxes.tolist(), cats.tolist(), scores.tolist())]


def _category_table(catIdx2id, device):
    """(device int64 table or None, host mapping or None) for to_json's category lookup: the COCO ids by default
    (utils/constants.py:2, COCO_CATEGORY_LIST[c]['id']); an integer list / dict becomes a device table, anything else
    (e.g. string ids) is mapped on the host from the class indices."""
    from .constants import COCO_CATEGORY_IDS
    src = COCO_CATEGORY_IDS if catIdx2id is None else catIdx2id
    try:
        if isinstance(src, dict):
            n = max(src) + 1
            vals = [int(src.get(i, -1)) for i in range(n)]
            if any(not isinstance(v, int) for v in src.values()):
                raise TypeError
        else:
            vals = [v for v in src]
            if any(not isinstance(v, int) for v in vals):
                raise TypeError
        key = (tuple(vals), str(device))
        hit = _category_table.cache.get(key)
        if hit is None:
            hit = torch.tensor(vals, dtype=torch.int64, device=device)
            _category_table.cache[key] = hit
        return hit, None
    except (TypeError, ValueError):
        return None, src


_category_table.cache = {}


def _json_rows(rows, cats, img_id, host_map):
    out = []
    for r, c in zip(rows, cats):
        out.append({'image_id': img_id, 'category_id': host_map[int(c)] if host_map is not None else c,
                    'bbox': r[:4], 'score': r[4]})
    return out


def batched_to_json(rec, img_ids, eval_type='x1y1wh', catIdx2id=None) -> list:
    '''
    `to_json` of every image of a batch of detection records (the concatenation the reference builds image by image,
    api/detection.py:67-74): one launch, one device->host copy.  img_ids: one id per image.
    '''
    if eval_type == 'cxcywhd':
        assert 'angle' in rec, "eval_type 'cxcywhd' needs rotated records"
        counts = ops.check_counts(rec['count'].cpu().tolist())
        bbox, angle = rec['bbox'].cpu(), rec['angle'].cpu()
        score, cls = rec['score'].cpu(), rec['class_idx'].cpu()
        out = []
        for b, (k, img_id) in enumerate(zip(counts, img_ids)):
            boxes = torch.cat([bbox[b, :k], angle[b, :k, None]], dim=1)
            out += _json_rotated(boxes, score[b, :k], cls[b, :k], img_id, catIdx2id)
        return out
    if eval_type != 'x1y1wh':
        raise NotImplementedError()
    table, host_map = _category_table(catIdx2id, rec['bbox'].device)
    rows, cat = ops.detections_to_json(rec['bbox'], rec['score'], rec['class_idx'], rec['count'], table)
    counts = ops.check_counts(rec['count'].cpu().tolist())
    rows, cat = rows.cpu(), cat.cpu()
    out = []
    for b, (k, img_id) in enumerate(zip(counts, img_ids)):
        out += _json_rows(rows[b, :k].tolist(), cat[b, :k].tolist(), img_id, host_map)
    return out


def batched_post_process(bboxes, cats, scores, conf_thres, nms_thres, records=None, rotated_nms=False, nms=None):
    '''
    The batched form of `for d in dts: d.post_process(...)` (examples/train.py:229-232):
    bboxes [B,N,4], cats [B,N], scores [B,N] on the device -> fixed-size records
    {count [B], bbox [B,512,4], class_idx [B,512], score [B,512], index [B,512]}, no host sync.
    bboxes [B,N,5] (cxcywhd) take the rotated kernel: rotated records, 'angle' [B,512] added.
    records: optional int32 [B, REC_WORDS] buffer (REC_ROT_WORDS for rotated boxes) to write (rows of a larger batch's
    record buffer).
    rotated_nms: the NMS compares the rotated rectangles (cxcywhd only; ValueError for [B,N,4]); same rotated records.
    nms: None, or an ops.Nms (class-agnostic suppression, Soft-NMS, box merging in the same launch; not with rotated_nms).
    '''
    return ops.postprocess(bboxes, cats, scores, conf_thres, nms_thres, TOPK, records=records, rotated_nms=rotated_nms, nms=nms)
