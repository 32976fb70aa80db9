"""API for the object detectors (reference: api/detection.py:19-205).

Same constructor and methods; the model forward and all post-processing run as HIP kernels
on the MI355X and only the surviving detections come back to the host.
"""
import collections
import os

import numpy as np
import PIL.Image
import torch

from .. import ops
from ..ops import Nms

from ..models.general import name_to_model
from ..utils import image_ops as imgUtils
from ..utils.structures import ImageObjects
from .appearance import Appearance
from .keyframes import KeyFrames
from .motion import CameraMotion
from .overlay import Overlay
from .zones import Zones


class Tiles:
    """Tiled ("sliced") detection on large frames, the `tiles=` argument of Detector.predict_frames and its YUV / json forms:
    the detector runs on overlapping windows of the frame at native resolution (ops.tile_windows: tiles of `size` = (h, w)
    or one int, clipped to the frame, `overlap` a fraction of the tile) and, with `full_frame`, on the whole frame as well;
    one more class-aware NMS on the device merges the windows' detections in frame coordinates (ops.merge_tile_records).
    nms_thres: the threshold of that merge (None: the call's nms_thres).  metric: its pair test, 'iou' or 'ios' --
    intersection over the smaller area, which also merges an object cut by a window seam with its whole view in the next
    window (not with rotated_nms)."""
    _align = 1                        # origins and sizes are multiples of this; the 4:2:0 methods use 2 at least

    def __init__(self, size, overlap=0.2, full_frame=True, nms_thres=None, metric='iou'):
        self.size = (int(size), int(size)) if isinstance(size, int) else tuple(int(v) for v in size)
        if len(self.size) != 2 or min(self.size) < 1:
            raise ValueError(f'Tiles: size = (h, w) with positive entries expected, got {size!r}')
        if not 0 <= overlap < 1:
            raise ValueError(f'Tiles: overlap {overlap!r} is outside [0, 1)')
        ops.merge_metric_id(metric)
        self.overlap, self.full_frame, self.metric = float(overlap), bool(full_frame), metric
        self.nms_thres = None if nms_thres is None else float(nms_thres)

    def __repr__(self):
        return (f'Tiles({self.size}, overlap={self.overlap}, full_frame={self.full_frame}, nms_thres={self.nms_thres}, '
                f'metric={self.metric!r})')


class Augment:
    """Test-time augmentation, the `augment=` argument of every Detector method that detects: the detector runs on mirrored and
    rescaled views of each frame and ONE fusion on the device turns what the views find into the frame's detections
    (ops.fuse_view_records; include/mydet.h: mydet_fuse_view_records_f32).  The views are the cross product of `scales` with
    the flips '' , 'h' (hflip), 'v' (vflip) and 'hv' (both), in that order -- or `views` = ((scale, flip), ...) says them
    one by one; YOLOv5's augment=True is ((1.0, ''), (0.83, 'h'), (0.67, '')).  At most 8 views, none twice, scales > 0.
    A view of scale s runs at input_size_s = max(div, round(input_size * s / div) * div) with div the model's input
    divisibility; scale 1.0 runs at the call's input_size itself.  A mirrored view is read in place by its input launch.
    fuse: 'nms' -- one more NMS over the views' boxes, as Tiles merges windows (metric 'iou' or 'ios') -- or 'wbf', Weighted
    Boxes Fusion ('cxcywh' models, metric 'iou'): the boxes of one object become their score-weighted mean, and a cluster
    found by n of V views scores mean * min(n, V) / V; clusters below min_score (default 0) are dropped.  thres: the overlap
    above which two boxes are one object (None: the call's nms_thres)."""

    def __init__(self, hflip=True, vflip=False, scales=(1.0,), fuse='nms', thres=None, metric='iou', min_score=None, views=None):
        if not isinstance(fuse, str) or fuse not in ops.FUSE_KINDS:
            raise ValueError(f'Augment: fuse {fuse!r} is not one of {sorted(ops.FUSE_KINDS)}')
        ops.merge_metric_id(metric)
        if fuse == 'wbf' and metric != 'iou':
            raise ValueError(f"Augment: fuse 'wbf' takes metric 'iou', not {metric!r}")
        if views is None:
            flips = [''] + (['h'] if hflip else []) + (['v'] if vflip else []) + (['hv'] if hflip and vflip else [])
            views = [(s, f) for s in (scales if isinstance(scales, (tuple, list)) else (scales,)) for f in flips]
        plan = []
        for view in views:
            try:
                scale, flip = view
                scale = float(scale)
            except (TypeError, ValueError):
                raise ValueError(f'Augment: a view is (scale, flip), got {view!r}') from None
            if not 0.0 < scale < float('inf'):
                raise ValueError(f'Augment: a positive finite scale expected, got {scale!r}')
            plan.append((scale, ops.view_flip_bits(flip, 'Augment')))
        if not 1 <= len(plan) <= ops.VIEWS_MAX:
            raise ValueError(f'Augment: 1..{ops.VIEWS_MAX} views expected, got {len(plan)}')
        if len(set(plan)) != len(plan):
            raise ValueError(f'Augment: a view is given twice in {plan}')
        if min_score is not None and not float(min_score) >= 0.0:
            raise ValueError(f'Augment: min_score >= 0 expected, got {min_score!r}')
        self.views = tuple(plan)                                     # ((scale, MYDET_VIEW_* bits), ...)
        self.fuse, self.metric = fuse, metric
        self.thres = None if thres is None else float(thres)
        self.min_score = 0.0 if min_score is None else float(min_score)

    def __repr__(self):
        names = {0: '', 1: 'h', 2: 'v', 3: 'hv'}
        return (f'Augment(views={tuple((s, names[f]) for s, f in self.views)}, fuse={self.fuse!r}, thres={self.thres}, '
                f'metric={self.metric!r}, min_score={self.min_score})')

    def plan(self, input_size, div, preprocessing):
        """[(input size of the view, flip bits)] for a call with `input_size` under `preprocessing` and a model whose input
        sizes are multiples of `div`.  'pad_divisible' has no input size: a scale other than 1.0 is a ValueError there."""
        out = []
        for scale, flip in self.views:
            size = input_size
            if scale != 1.0:
                if preprocessing == 'pad_divisible' or input_size is None:
                    raise ValueError(f"augment: a view of scale {scale} needs a preprocessing with an input_size, not {preprocessing!r}")
                size = max(int(div), int(round(input_size * scale / div)) * int(div))
            out.append((size, flip))
        return out


class Draw:
    """The settings of Detector.annotate_frames and its YUV forms: what the overlay renderer paints (ops.draw_boxes;
    include/mydet.h has the raster rules).  thickness: the outline's, 1..64 pixels; None = max(1, round(H / 360)) for frames
    of H rows (the reference's line_width).  labels: any of 'class', 'score', 'id' ('id' shows with a tracker only).
    label_height: rows of a label cell, 8..64; None = round(H / 45) kept inside 10..64.  fill_alpha: 0 (no fill) .. 255.
    color_by: 'class', 'id' or None = 'id' with a tracker and 'class' without; color: one (r, g, b) for every box instead.
    class_names: a list of ASCII names for the class part (16 characters are shown); None = the class index."""

    def __init__(self, thickness=None, labels=('class', 'score'), label_height=None, fill_alpha=0, color_by=None, color=None,
                 class_names=None):
        if color_by is not None and (not isinstance(color_by, str) or color_by not in ('class', 'id')):
            raise ValueError(f"Draw: color_by {color_by!r} is not 'class', 'id' or None")
        # ops.draw_style has the rules; None entries are checked with a stand-in and resolved per frame size
        ops.draw_style(2 if thickness is None else thickness, fill_alpha, color_by or 'class', color, labels,
                       16 if label_height is None else label_height, class_names)
        self.thickness, self.label_height, self.fill_alpha = thickness, label_height, fill_alpha
        self.labels = (labels,) if isinstance(labels, str) else tuple(labels or ())
        self.color_by, self.color = color_by, color
        self.class_names = None if class_names is None else list(class_names)
        self._styles = {}

    def __repr__(self):
        return (f'Draw(thickness={self.thickness}, labels={self.labels}, label_height={self.label_height}, fill_alpha={self.fill_alpha}, '
                f'color_by={self.color_by!r}, color={self.color}, class_names={None if self.class_names is None else len(self.class_names)})')

    def style(self, frame_hw, tracked=False):
        """The ops.DrawStyle for frames of size frame_hw (cached: its device tables are made once)."""
        from ..utils.visualization import default_label_height
        h = int(frame_hw[0])
        key = (max(1, round(h / 360)) if self.thickness is None else self.thickness,
               default_label_height(h) if self.label_height is None else self.label_height,
               self.color_by or ('id' if tracked else 'class'))
        if key not in self._styles:
            self._styles[key] = ops.draw_style(min(key[0], 64), self.fill_alpha, key[2], self.color, self.labels, key[1], self.class_names)
        return self._styles[key]


class Redact:
    """The settings of Detector.redact_frames and its YUV forms, and the `redact=` argument of annotate_frames*: how the detections
    are hidden in the frames before they leave the device (ops.redact_boxes; include/mydet.h has the rules).  mode: 'mosaic'
    (pixelate: a covered pixel becomes the mean of its cell), 'smooth' (the bilinear interpolation of the cell means: a strong
    blur whose cost does not depend on its radius) or 'solid' (`color`).  cell: the cell size, even, 4..64; None =
    min(64, max(4, 2 * ((min(H, W) + 48) // 96))) for frames of H x W (22 at 1080p).  shape: 'box' or 'ellipse'.  pad: the box is
    scaled by it first (1.25 = a quarter more), finite and > 0.  classes: None = every detection, or 1..16 class indices = only
    those (people but not cars).  color: the (r, g, b) of 'solid'."""

    def __init__(self, mode='mosaic', cell=None, shape='box', pad=1.0, classes=None, color=(0, 0, 0)):
        # ops.redact_style has the rules; a None cell is checked with a stand-in and resolved per frame size
        checked = ops.redact_style(mode, 16 if cell is None else cell, shape, pad, classes, color)
        self.mode, self.cell, self.shape, self.pad, self.classes, self.color = mode, cell, shape, checked.pad, checked.classes, checked.color
        self._styles = {}

    def __repr__(self):
        return (f'Redact(mode={self.mode!r}, cell={self.cell}, shape={self.shape!r}, pad={self.pad}, classes={self.classes}, '
                f'color={self.color})')

    @staticmethod
    def default_cell(frame_hw):
        """The cell size of cell=None for frames of size frame_hw: about 1 / 48 of the shorter side, even, inside 4..64."""
        return min(64, max(4, 2 * ((min(int(frame_hw[0]), int(frame_hw[1])) + 48) // 96)))

    def style(self, frame_hw):
        """The ops.RedactStyle for frames of size frame_hw (cached)."""
        cell = self.default_cell(frame_hw) if self.cell is None else self.cell
        if cell not in self._styles:
            self._styles[cell] = ops.redact_style(self.mode, cell, self.shape, self.pad, self.classes, self.color)
        return self._styles[cell]


class Chips:
    """The settings of Detector.crop_frames and its YUV forms: the image of every detected object, cut out of the frame, turned
    upright and resampled to one size on the device (ops.crop_boxes; include/mydet.h has the sampling rules).  size: (height,
    width) of a chip, each 1..256.  pad: the box is scaled by it before it is cut out (1.2 = 20 % context), finite and > 0.
    max_per_frame: chip slots per frame, 1..512; a frame with more objects gets chips for its first max_per_frame rows.  out:
    'input' = float32 [3,h,w] chips, / 255 and normalised by the model's own input_format (what a classifier on the same
    preprocessing takes); 'uint8' = [h,w,3] pixels.  fill: the (r, g, b) of everything outside the frame."""

    def __init__(self, size=(128, 64), pad=1.0, max_per_frame=64, out='input', fill=(0, 0, 0)):
        if max_per_frame is None:
            raise ValueError('Chips: max_per_frame is an int in 1..512, got None')
        (self.size, self.max_per_frame, self.pad, self.fill, _, _) = ops.crop_settings('Chips', size, max_per_frame, pad, fill, out, None)
        self.out = out

    def __repr__(self):
        return f'Chips(size={self.size}, pad={self.pad}, max_per_frame={self.max_per_frame}, out={self.out!r}, fill={self.fill})'

    def kwargs(self, input_format):
        """The keyword arguments of the ops.crop_* functions for a model of `input_format`."""
        return dict(size=self.size, max_per_frame=self.max_per_frame, pad=self.pad, fill=self.fill, out=self.out, input_format=input_format)


# what the keyword arguments of a frame method say (Detector._call_settings reads them, nothing else does)
_Call = collections.namedtuple('_Call', 'preprocessing input_size conf_thres nms_thres rotated_nms nms tiles whole augment')


class _Frames:
    """B frames of one size for the frame methods of Detector `det`: what differs by pixel format, and nothing else.  The
    constructors make the host-side checks and set n (= B), hw = (H, W) and idxs, the frames' places in the call's list; no
    device is touched before on_device(), which moves the frames to the model's device once.  Subclasses give on_device(),
    input(), align() (of a Tiles' windows), image() -> (what the ops.draw_* / ops.crop_* functions take first, their layout
    keywords) and drawn()."""

    def device(self):
        return next(self.det.model.parameters()).device

    def draw(self, found, style):
        """Paint `found` -- a record dict, read in place, or a list of ImageObjects, one per frame -- into the frames; returns
        what annotate_frames* returns as `drawn`."""
        from ..utils.visualization import objects_to_rows
        image, yuv = self.image()
        if isinstance(found, dict):
            ops.draw_records(image, found, style, **yuv)
        else:
            boxes, counts, scores, classes, ids = objects_to_rows(found, self.device())
            (ops.draw_boxes_yuv420 if yuv else ops.draw_boxes)(image, boxes=boxes, style=style, counts=counts, scores=scores, classes=classes,
                                                               ids=ids, **yuv)
        return self.drawn()

    def redact(self, found, style):
        """Hide `found` (as in draw) in the frames; returns what redact_frames* returns as `redacted`."""
        from ..utils.visualization import objects_to_rows
        image, yuv = self.image()
        if isinstance(found, dict):
            ops.redact_records(image, found, style, **yuv)
        else:
            boxes, counts, _, classes, _ = objects_to_rows(found, self.device())
            (ops.redact_boxes_yuv420 if yuv else ops.redact_boxes)(image, boxes=boxes, style=style, counts=counts, classes=classes, **yuv)
        return self.drawn()

    def crop(self, found, chip_kwargs):
        """The chip buffer [B,M,...] of `found` (as in draw); chip_kwargs: Chips.kwargs(...)."""
        from ..utils.visualization import objects_to_rows
        image, yuv = self.image()
        if isinstance(found, dict):
            return ops.crop_records(image, found, **yuv, **chip_kwargs)
        boxes, counts = objects_to_rows(found, self.device())[:2]
        return (ops.crop_boxes_yuv420 if yuv else ops.crop_boxes)(image, boxes=boxes, counts=counts, **yuv, **chip_kwargs)


def _frame_subset(t, idxs):
    """Frames `idxs` (ascending, at least one) of a device tensor [B, ...]: a view when they are evenly spaced, else one gather."""
    step = idxs[1] - idxs[0] if len(idxs) > 1 else 1
    if all(b - a == step for a, b in zip(idxs, idxs[1:])):
        return t[idxs[0]:idxs[-1] + 1:step]
    return t.index_select(0, torch.tensor(idxs, device=t.device))


class _RgbFrames(_Frames):
    """uint8 RGB frames [B,H,W,3]: the tensors `parts` of one size from Detector._frame_groups.  packed: the call goes on to
    draw into or read the frames, which takes packed pixels -- frames that are not are copied once, on the device."""

    def __init__(self, det, idxs, parts, packed=False):
        self.det, self.idxs, self.parts, self.packed = det, idxs, parts, packed
        self.n, self.hw, self.frames = len(idxs), (int(parts[0].shape[1]), int(parts[0].shape[2])), None

    def on_device(self):
        if self.frames is None:
            dev, parts = self.device(), self.parts
            if len(parts) > 1:                                       # a list: gather it where it already is
                where = dev if all(t.device == dev for t in parts) else torch.device('cpu')
                parts = [torch.cat([t.to(where) for t in parts])]
            self.frames = parts[0].to(dev, non_blocking=True)
            if self.packed and not ops.packed_pixels(self.frames):
                self.frames = self.frames.contiguous()
        return self.frames

    def input(self, geometry, out=None, window=None, flip=0):
        """The float32 network input of the frames, or of their crop view at window = (y0, x0, h, w), or of their mirrored
        view `flip` (ops.view_flip_bits): one launch."""
        fr = self.on_device()
        if window is not None:
            y0, x0, h, w = window
            fr = fr[:, y0:y0 + h, x0:x0 + w]
        return ops.frames_to_input(fr, geometry, self.det.model.input_format, out=out, flip=flip)

    def align(self, tiles):
        return tiles._align

    def image(self):
        return self.on_device(), {}

    def select(self, idxs):
        """The source of frames `idxs` (ascending) of this one, on the device: a strided view when they are evenly spaced, else
        one gather of those frames."""
        return _RgbFrames(self.det, list(range(len(idxs))), [_frame_subset(self.on_device(), idxs)])

    drawn = on_device


class _Yuv420Frames(_Frames):
    """The planes of 4:2:0 frames of `layout` with their matrix and range; planes as Detector._yuv_planes takes them.
    drawn_by: the method that goes on to draw into the planes (8-bit layouts only; a single surface then stays one tensor,
    which is what comes back as `drawn`)."""

    def __init__(self, det, planes, layout, matrix, full_range, drawn_by=None):
        if ops.yuv420_layout(layout)[1] != 1 and drawn_by is not None:
            raise ValueError(f'{drawn_by}: layout {layout!r} is not drawn into; the 8-bit layouts nv12, nv21, i420 and yv12 are')
        ops.yuv_matrix_id(matrix)
        y = det._yuv_planes(planes, layout)[0]                       # the checks alone: no device is touched
        self.det, self.given, self.yuv, self.in_place = det, planes, dict(layout=layout, matrix=matrix, full_range=full_range), drawn_by is not None
        self.n, self.hw, self.idxs = int(y.shape[0]), (int(y.shape[1]), int(y.shape[2])), list(range(y.shape[0]))
        self.planes = self.surface = None

    def on_device(self):
        if self.planes is None:
            dev, given = self.device(), self.given
            if self.in_place and isinstance(given, (np.ndarray, torch.Tensor)):
                given = (torch.from_numpy(np.ascontiguousarray(given)) if isinstance(given, np.ndarray) else given).to(dev, non_blocking=True)
                if not (given[0] if given.dim() == 3 else given).is_contiguous():
                    given = given.contiguous()                       # the planar split needs packed rows to stay a view
                self.surface = given
            self.planes = tuple(self.det._yuv_planes(given, self.yuv['layout'], device=dev))
        return self.planes

    def input(self, geometry, out=None, window=None, flip=0):
        """As _RgbFrames.input; a window with even origin and size is itself a 4:2:0 frame."""
        ts = self.on_device()
        if window is not None:
            y0, x0, h, w = window
            ts = [ts[0][:, y0:y0 + h, x0:x0 + w]] + [t[:, y0 // 2:(y0 + h) // 2, x0 // 2:(x0 + w) // 2] for t in ts[1:]]
        return ops.yuv420_to_input(ts, self.yuv['layout'], geometry, self.det.model.input_format, self.yuv['matrix'], self.yuv['full_range'], out=out,
                                   flip=flip)

    def align(self, tiles):
        return tiles._align * (2 if tiles._align % 2 else 1)

    def image(self):
        return self.on_device(), self.yuv

    def select(self, idxs):
        """As _RgbFrames.select, of every plane."""
        sub = object.__new__(_Yuv420Frames)
        sub.det, sub.given, sub.yuv, sub.in_place, sub.surface = self.det, None, self.yuv, False, None
        sub.n, sub.hw, sub.idxs = len(idxs), self.hw, list(range(len(idxs)))
        sub.planes = tuple(_frame_subset(t, idxs) for t in self.on_device())
        return sub

    def drawn(self):
        return self.on_device() if self.surface is None else self.surface


class Detector():
    '''Wrapper for image object detectors

    Args:
        model_name: str, see mydetection_amd.configs.NAMES for available names
        model_and_cfg: (model, cfg) built elsewhere
        weights_path: checkpoint with a 'model' state_dict (reference key names)
        cpu: must be False -- this package has no CPU path
        nms: None, or an Nms: how the post-process suppresses in every call that does not say otherwise (`nms=` per call)
        augment: None, or an Augment: test-time augmentation in every call that does not say otherwise (`augment=` per call)
    '''
    def __init__(self, model_name: str = None, model_and_cfg: tuple = None,
                 weights_path: str = None, cpu=False, nms=None, augment=None):
        if cpu:
            raise RuntimeError('mydetection_amd.Detector(cpu=True): there is no CPU path; '
                               'use the reference for CPU inference')
        if model_and_cfg:
            self.model, cfg = model_and_cfg
        else:
            self.model, cfg = name_to_model(model_name)
            self.model.eval()
            self.model = self.model.cuda()

        self._init_preprocess(cfg)
        self._init_postprocess(cfg)
        self.nms = self._nms_setting(nms, self.conf_thres, self.rotated_nms)
        self.augment = self._augment_setting(augment, None, self.rotated_nms, self.preprocess, self.input_size)

        n_params = sum(p.numel() for p in self.model.parameters() if p.requires_grad)
        print('Number of parameters:', n_params)
        if weights_path:
            self.model.load_state_dict(torch.load(weights_path)['model'])
        self.on_cpu = False
        # hipGraph replay of forward + post-process per (batch, H, W, conf, nms), captured the second time a shape is seen
        # (a one-off shape is not worth two warm-up passes); MYDET_GRAPH=0 keeps every call eager
        self.use_graph = os.environ.get('MYDET_GRAPH', '1') != '0'
        from ..graph import GraphCache
        self._graphs = GraphCache(int(os.environ.get('MYDET_MAX_GRAPHS', self._MAX_GRAPHS)))

    def _init_preprocess(self, cfg):
        self.divisibe = cfg['general.input_divisibility']
        self.input_size = cfg.get('test.default_input_size', None)
        self.preprocess = cfg['test.preprocessing']

    def _init_postprocess(self, cfg):
        self.conf_thres = cfg['test.default_conf_thres']
        self.nms_thres = cfg['test.nms_thres']
        # opt-in: NMS on the rotated rectangles of a 'cxcywhd' model (no shipped config sets the key: the default is the
        # axis-aligned NMS the reference runs); the `rotated_nms` keyword of the predict methods overrides it per call
        self.rotated_nms = bool(cfg.get('test.rotated_nms', False))

    def _nms_setting(self, nms, conf_thres, rotated_nms):
        """An `nms=` argument checked against this model and the thresholds it will run with (ops.nms_mode has the rules;
        no device is touched).  Returns it."""
        ops.nms_mode('Detector', nms, conf_thres, 5 if self.model.bb_format == 'cxcywhd' else 4, rotated_nms)
        return nms

    def _augment_setting(self, augment, tiles, rotated_nms, preprocessing, input_size):
        """An `augment=` argument checked against this model and the call it will run in; no device is touched.  Returns it."""
        if augment is None:
            return None
        if not isinstance(augment, Augment):
            raise TypeError(f'augment: a mydetection_amd.api.Augment (or None) expected, got {type(augment).__name__}')
        if tiles is not None:
            raise ValueError('augment: test-time augmentation of a tiled call is not provided; give tiles= or augment=')
        if augment.fuse == 'wbf' and self.model.bb_format == 'cxcywhd':
            raise ValueError("augment: fuse 'wbf' is defined for 'cxcywh' models only (no mean of angles); this one predicts 'cxcywhd'")
        if augment.fuse == 'wbf' and rotated_nms:
            raise ValueError("augment: fuse 'wbf' is not defined with rotated_nms")
        if augment.metric == 'ios' and rotated_nms:
            raise ValueError("augment: metric 'ios' is defined for the axis-aligned test only, not with rotated_nms")
        augment.plan(input_size, self.divisibe, preprocessing)
        return augment

    def evaluation_predict(self, eval_info: dict, **kwargs):
        '''
        COCO-style detections of a whole evaluation set (reference: api/detection.py:58-76, a per-image loop).
        Images are decoded on the host and then handled `batch_size` (default 16) at a time: device resize + pad +
        normalise, ONE forward and ONE batched post-process per group of equal input size, boxes mapped back and
        converted to json rows on the device.  The list has the reference's order (image by image).
        '''
        img_dir = eval_info['image_dir']
        infos = list(eval_info['image_info']['images'])
        kwargs = dict(kwargs)
        batch_size = int(kwargs.pop('batch_size', 16))
        cat_map = kwargs.pop('catIdx2id', None)
        detection_json = []
        for i in range(0, len(infos), batch_size):
            chunk = infos[i:i + batch_size]
            imgs = [imgUtils.imread_pil(os.path.join(img_dir, info['file_name'])) for info in chunk]
            detection_json += self._json_batch(imgs, [info['id'] for info in chunk], eval_info['eval_type'], cat_map, **kwargs)
        return detection_json

    def predict_imgDir(self, img_dir, **kwargs):
        """reference: api/detection.py:93-110 (per-image loop); batched like evaluation_predict."""
        kwargs = dict(kwargs)
        batch_size = int(kwargs.pop('batch_size', 16))
        names = os.listdir(img_dir)
        detection_json = []
        for i in range(0, len(names), batch_size):
            chunk = names[i:i + batch_size]
            ids = []
            for imname in chunk:
                assert imname[-4] == '.'
                ids.append(int(imname[:-4]) if imname[:-4].isdigit() else imname[:-4])
            imgs = [imgUtils.imread_pil(os.path.join(img_dir, n)) for n in chunk]
            detection_json += self._json_batch(imgs, ids, 'x1y1wh', None, **kwargs)
        return detection_json

    def _json_batch(self, pil_imgs, img_ids, eval_type, cat_map, **kwargs):
        from ..utils.structures import batched_to_json
        out = [None] * len(pil_imgs)
        for idxs, rec in self._records_by_size(pil_imgs, **kwargs):
            rows = batched_to_json(rec, [img_ids[j] for j in idxs], eval_type, cat_map)
            counts = ops.check_counts(rec['count'].cpu().tolist())
            o = 0
            for j, k in zip(idxs, counts):
                out[j] = rows[o:o + k]
                o += k
        return [d for per_img in out for d in per_img]

    def detect_one(self, **kwargs):
        '''
        object detection in one single image: (img_path: str) or (pil_img: PIL.Image);
        see _predict_pil() for the optional arguments.  return_img=True returns the image as a numpy array with the detections
        drawn on it (ImageObjects.draw_on_np, the overlay renderer on the device), as the reference does; the drawing
        keywords of utils.visualization.draw_bboxes_on_np are passed on.  show_img (a matplotlib window) is not provided.
        '''
        assert 'pil_img' in kwargs or 'img_path' in kwargs
        img = kwargs.pop('pil_img', None) or imgUtils.imread_pil(kwargs.pop('img_path'))
        if kwargs.get('show_img', False):
            raise NotImplementedError('show_img opens a window; use return_img=True and show the array')
        draw_kw = {k: kwargs.pop(k) for k in ('color', 'line_width', 'put_text', 'show_class', 'class_names', 'label_height', 'fill_alpha')
                   if k in kwargs}
        if kwargs.pop('return_img', False):
            detections = self._predict_pil(img, **kwargs)
            np_img = np.array(img.convert('RGB'))
            detections.draw_on_np(np_img, class_map='COCO', **draw_kw)
            return np_img
        return self._predict_pil(img, **kwargs)

    def _predict_pil(self, pil_img, **kwargs):
        '''
        Args:
            pil_img, preprocessing (str), input_size (int), conf_thres (float), nms_thres (float), rotated_nms (bool),
            nms (an Nms or None: class-agnostic suppression, Soft-NMS or box merging; the detector's own by default),
            augment (an Augment or None: test-time augmentation; the detector's own by default.  The image's pixels then
            take the frame path: predict_frames on np.asarray(img.convert('RGB')))
        '''
        assert isinstance(pil_img, PIL.Image.Image), 'input must be a PIL.Image'
        return self.predict_batch([pil_img], **kwargs)[0]

    def _geometry(self, ori_h, ori_w, pre_proc_name, input_size=None):
        """What api/detection.py:177-205 does to an image of (ori_h, ori_w), as numbers: the resize target (h, w) or
        None, the (top, left) offset of the resized image inside the network input, the input size (H, W), and
        pad_info for bboxes_to_original_ (None when the boxes are already in image coordinates)."""
        assert isinstance(self.divisibe, int)
        div = self.divisibe

        def up(v):
            return int(np.ceil(v / div) * div)
        if pre_proc_name == 'pad_divisible':
            return None, (0, 0), (up(ori_h), up(ori_w)), None
        if pre_proc_name == 'resize_pad_divisible':
            assert input_size is not None
            factor = input_size / max(ori_h, ori_w)                  # utils/image_ops.py:30-33 (resize_pil, shorter=False)
            th, tw = round(ori_h * factor), round(ori_w * factor)
            return (th, tw), (0, 0), (up(th), up(tw)), (ori_w, ori_h, 0, 0, tw, th)
        if pre_proc_name == 'resize_pad_square':
            assert input_size is not None
            scale = input_size / max(ori_w, ori_h)                   # utils/image_ops.py:55-137 (rect_to_square, aug=False)
            rw, rh = int(ori_w * scale), int(ori_h * scale)
            left, top = (input_size - rw) // 2, (input_size - rh) // 2
            return (rh, rw), (top, left), (input_size, input_size), (ori_w, ori_h, left, top, rw, rh)
        raise Exception('Unknown preprocessing name')

    def preprocess_batch(self, pil_imgs, **kwargs):
        """Network inputs of a list of PIL images, grouped by input size: yields (indices, x [n,3,H,W] float32 on the
        device, pad_infos, image sizes).  Per image the host only decodes the file; resize (PIL-exact: the reference's
        tvf.resize of a PIL image), zero padding, /255 and normalisation (api/detection.py:158-163) are HIP kernels on
        the uint8 pixels."""
        pre_proc = kwargs.get('preprocessing', self.preprocess)
        input_size = kwargs.get('input_size', self.input_size)
        groups = {}
        for j, img in enumerate(pil_imgs):
            assert isinstance(img, PIL.Image.Image), 'input must be a PIL.Image'
            geo = self._geometry(img.height, img.width, pre_proc, input_size)
            groups.setdefault(geo[2], []).append((j, img, geo))
        dev = next(self.model.parameters()).device
        for (Hp, Wp), items in groups.items():
            buf = torch.zeros((len(items), Hp, Wp, 3), dtype=torch.uint8, device=dev)     # zero padding lives here
            for n, (j, img, (target, (top, left), _, _)) in enumerate(items):
                u8 = torch.from_numpy(np.array(img.convert('RGB'), dtype=np.uint8)).to(dev, non_blocking=True)
                ops.resize_bilinear_u8(u8, target or (img.height, img.width), buf[n], top, left)
            x = ops.preprocess_u8(buf, (Hp, Wp), self.model.input_format)
            yield ([j for j, _, _ in items], x, [g[3] for _, _, g in items],
                   [(img.height, img.width) if g[3] is not None else (Hp, Wp) for _, img, g in items])

    def _records_by_size(self, pil_imgs, **kwargs):
        """Detection records of a list of PIL images, grouped by network input size: yields (indices, records) with the
        boxes already in the coordinates of the original images.  With augment= the pixels of the images take the frame
        path (whose plain form equals this one): one augmented call per image size."""
        if kwargs.get('augment', self.augment) is not None:
            yield from self._frame_records([np.array(img.convert('RGB')) for img in pil_imgs], **kwargs)
            return
        conf_thres = kwargs.get('conf_thres', self.conf_thres)
        nms_thres = kwargs.get('nms_thres', self.nms_thres)
        rotated_nms = bool(kwargs.get('rotated_nms', self.rotated_nms))
        if rotated_nms and self.model.bb_format != 'cxcywhd':
            raise ValueError(f"rotated_nms needs a 'cxcywhd' model; this one predicts {self.model.bb_format!r}")
        nms = self._nms_setting(kwargs.get('nms', self.nms), conf_thres, rotated_nms)
        for idxs, x, pads, hws in self.preprocess_batch(pil_imgs, **kwargs):
            rec = self._records(x, conf_thres, nms_thres, rotated_nms, nms)
            if any(p is not None for p in pads):
                ops.records_to_original_(rec, pads)
            rec['img_hw'] = hws
            yield idxs, rec

    _MAX_GRAPHS = 6
    augment = None                    # the default of `augment=`; __init__ sets the detector's own

    def reset_graphs(self):
        """Forget every captured hipGraph (after editing parameters in place, or to release the graphs' activation pools)."""
        self._graphs.clear()

    def _records(self, x, conf_thres, nms_thres, rotated_nms=False, nms=None):
        """Detection records of one network input batch (boxes in network-input coordinates): a hipGraph replay when
        this (shape, thresholds, kind of NMS, NMS mode) has been seen before, the eager launch sequence otherwise."""
        from ..utils.structures import batched_post_process
        key = (tuple(x.shape), float(conf_thres), float(nms_thres), bool(rotated_nms))
        if nms is not None:                                          # an Nms hashes by value; without one the key is what it was
            key += (nms,)
        if self.use_graph:
            cache = self._graphs
            g = cache.lookup(key)                                    # LRU; drops a graph captured before a weight change
            if g is None and cache.should_capture(key):
                from ..graph import GraphedPath
                # each graph owns its activations; the lane count is the detector's (below), not a timing decision
                g = cache.insert(key, GraphedPath(self.model, x, conf_thres, nms_thres, lanes=self.batch_lanes(x.shape[0]),
                                                      rotated_nms=rotated_nms, nms=nms))
            if g is not None:
                return {k: v.clone() for k, v in g(x).items()}       # the graph's own record buffers are overwritten by the next replay
            cache.note_eager(key)
        with torch.no_grad():
            lanes = self.batch_lanes(x.shape[0])
            if lanes == 1:
                bb, ci, sc = self.model.forward_candidates(x)
                return batched_post_process(bb, ci, sc, conf_thres, nms_thres, rotated_nms=rotated_nms, nms=nms)
            # the eager form of a laned graph: the same parts of the batch, one after the other -- bit-identical to the replay
            words = ops.record_words(getattr(self.model, 'bbox_param', 4))
            records = torch.empty((x.shape[0], words), dtype=torch.int32, device=x.device)
            lo = 0
            for part in x.tensor_split(lanes):
                bb, ci, sc = self.model.forward_candidates(part)
                batched_post_process(bb, ci, sc, conf_thres, nms_thres, records=records[lo:lo + part.shape[0]], rotated_nms=rotated_nms,
                                     nms=nms)
                lo += part.shape[0]
            return ops.record_views(records)

    def batch_lanes(self, batch):
        """How many parts a batch of this size is evaluated in (graph.GraphedPath: parallel graph branches).  A fixed rule
        -- MYDET_LANES when it is a number, else the model's `batch_lanes_hint` (2 for the EfficientNet-based models,
        whose step is many short launches; 1 for Darknet-53) for even batches -- so that the eager calls that precede a
        capture and the replays that follow it give the same bits."""
        env = os.environ.get('MYDET_LANES', 'auto')
        want = int(env) if env.isdigit() else int(getattr(self.model, 'batch_lanes_hint', 1))
        if want <= 1 or batch < 2:
            return 1
        return min(want, batch) if env.isdigit() else (want if batch % want == 0 else 1)

    @staticmethod
    def _uint8_tensor(f, what):
        """f, a torch.uint8 tensor or numpy.uint8 array, as a tensor (no copy of a contiguous array); a TypeError worded with
        `what` (the caller and the argument) for any other type or dtype."""
        if not isinstance(f, (np.ndarray, torch.Tensor)):
            raise TypeError(f'{what}: a uint8 torch.Tensor or numpy.ndarray expected, got {type(f).__name__}')
        is_np = isinstance(f, np.ndarray)
        if f.dtype != (np.uint8 if is_np else torch.uint8):
            raise TypeError(f"{what}: uint8 expected, got a {'numpy array' if is_np else 'tensor'} of dtype {f.dtype}")
        return torch.from_numpy(np.ascontiguousarray(f)) if is_np else f

    @staticmethod
    def _frame_groups(frames):
        """Frames as uint8 tensors grouped by size: (number of frames, [(indices, [tensors [n,H,W,3]])]).  Accepts a
        torch.uint8 tensor or numpy.uint8 array of shape [B,H,W,3] or [H,W,3], on the host or the device, or a list of them;
        anything else is a TypeError (type, dtype) or a ValueError (shape).  Touches no device."""
        items = list(frames) if isinstance(frames, (list, tuple)) else [frames]
        groups, n = {}, 0
        for f in items:
            t = Detector._uint8_tensor(f, 'predict_frames: frames (or a list of them)')
            if f.ndim not in (3, 4) or f.shape[-1] != 3 or min(f.shape) < 1:
                raise ValueError(f'predict_frames: frames of shape [B,H,W,3] or [H,W,3] expected, got {tuple(f.shape)}')
            t = t.unsqueeze(0) if t.dim() == 3 else t
            idxs, parts = groups.setdefault((t.shape[1], t.shape[2]), ([], []))
            idxs += range(n, n + t.shape[0])
            parts.append(t)
            n += t.shape[0]
        return n, list(groups.values())

    def _rgb_sources(self, frames, what=None):
        """The frame sources of uint8 RGB frames (_frame_groups: host checks only), one per frame size.  what: the method that
        goes on to draw into or cut chips out of the frames -- frames of one size (ValueError), packed on the device."""
        _, groups = self._frame_groups(frames)
        if what is not None and len(groups) != 1:
            raise ValueError(f'{what}: frames of one size expected, got {[tuple(parts[0].shape[1:3]) for _, parts in groups]}')
        return [_RgbFrames(self, idxs, parts, packed=what is not None) for idxs, parts in groups]

    @staticmethod
    def _one_source(sources, kind):
        if len(sources) != 1:
            raise ValueError(f'predict_frames: a {kind} call takes frames of one size, got {[src.hw for src in sources]}')
        return sources[0]

    def _call_settings(self, kwargs, whole=False):
        """What the keyword arguments of a frame method say, read once (a _Call), with the argument rules that need no frame
        and no device.  whole: the records are wanted as the views of ONE buffer (the tests' `_whole_records` asks for it too)."""
        tiles = kwargs.get('tiles')
        if tiles is not None and not isinstance(tiles, Tiles):
            raise TypeError(f'tiles: a mydetection_amd.api.Tiles (or None) expected, got {type(tiles).__name__}')
        rotated_nms = bool(kwargs.get('rotated_nms', self.rotated_nms))
        if tiles is not None and tiles.metric == 'ios' and rotated_nms:
            raise ValueError("tiles: metric 'ios' is defined for the axis-aligned test only, not with rotated_nms")
        if rotated_nms and self.model.bb_format != 'cxcywhd':
            raise ValueError(f"rotated_nms needs a 'cxcywhd' model; this one predicts {self.model.bb_format!r}")
        conf_thres = kwargs.get('conf_thres', self.conf_thres)
        nms = self._nms_setting(kwargs.get('nms', self.nms), conf_thres, rotated_nms)
        preprocessing, input_size = kwargs.get('preprocessing', self.preprocess), kwargs.get('input_size', self.input_size)
        augment = self._augment_setting(kwargs.get('augment', self.augment), tiles, rotated_nms, preprocessing, input_size)
        return _Call(preprocessing, input_size, conf_thres, kwargs.get('nms_thres', self.nms_thres), rotated_nms, nms, tiles,
                     bool(whole or kwargs.get('_whole_records')), augment)

    def _frame_records(self, frames, **kwargs):
        """Detection records of uint8 frames: yields (indices, records) per network input size, like _records_by_size (same
        batches in the same order, so the same bits).  tiles: a Tiles, or None (see predict_frames)."""
        return self._source_records(self._rgb_sources(frames), self._call_settings(kwargs))

    def _source_records(self, sources, call):
        """[(frame indices, records)] of frame sources, boxes in frame coordinates: per network input size, or, tiled, of the
        one source's frames after the merge; augmented, of each source's frames after the fusion of its views."""
        if call.augment is not None:
            return [pair for src in sources for pair in self._records_of_views(src, call)]
        if call.tiles is None:
            return self._records_of_inputs(sources, call)
        return self._records_of_windows(self._one_source(sources, 'tiled'), call)

    def _carried_records(self, src, call, keyframes, tracker, shift):
        """[(frame indices, records)] of the B frames of one source with keyframes=: only the key frames of the call (host
        arithmetic on the KeyFrames' counter) go through _source_records -- the forward pass, the post-process, the window merge,
        the view fusion --, as a subset of the source; then ONE launch pair (ops.carry_records) on the whole original frames makes
        the record of every frame: a key frame's is the detector's, copied, an in-between frame's the key boxes carried by their
        pixels.  shift: the camera motion of the call's frames, or None.  No host synchronisation."""
        B, S = src.n, tracker.streams
        F = B // S
        keys = [s * F + f for s in range(S) for f, k in enumerate(keyframes.key_mask(F)) if k]
        key_rec = None
        if keys:
            (_, key_rec), = self._source_records([src.select(keys)], call)
            hw = key_rec['img_hw'][0]
        else:                                                        # what the records of these frames would report
            geo = self._geometry(src.hw[0], src.hw[1], call.preprocessing, call.input_size)
            hw = src.hw if call.tiles is not None or geo[3] is not None else geo[2]
        rec = keyframes.run(*src.image(), key_rec, tracker, src.hw, F, 5 if self.model.bb_format == 'cxcywhd' else 4, shift)
        rec['img_hw'] = [hw] * B
        return [(list(range(B)), rec)]

    def _records_of_inputs(self, sources, call):
        """The untiled records: sources of one network input size are one batch, in input order (one fused launch per source
        builds its part: ops.frames_to_input / ops.yuv420_to_input), and yield one (indices, records)."""
        by_input = {}
        for src in sources:
            geo = self._geometry(src.hw[0], src.hw[1], call.preprocessing, call.input_size)
            by_input.setdefault(geo[2], []).append((src, geo))
        for members in by_input.values():
            idxs, xs, pads, hws = [], [], [], []
            for src, geo in members:
                xs.append(src.input(geo))
                idxs += src.idxs
                pads += [geo[3]] * src.n
                hws += [src.hw if geo[3] is not None else geo[2]] * src.n
            x = xs[0]
            if len(xs) > 1:                                          # several frame sizes, one input size: one batch, in input order
                order = sorted(range(len(idxs)), key=idxs.__getitem__)
                x = torch.cat(xs)[torch.tensor(order, device=x.device)]
                idxs, pads, hws = [idxs[k] for k in order], [pads[k] for k in order], [hws[k] for k in order]
            rec = self._records(x, call.conf_thres, call.nms_thres, call.rotated_nms, call.nms)
            if call.whole:                                           # the views of ONE buffer (a graph replay hands out copies)
                rec = ops.record_views(rec['records'])
            if any(p is not None for p in pads):
                ops.records_to_original_(rec, pads)
            rec['img_hw'] = hws
            yield idxs, rec

    def _records_of_windows(self, src, call):
        """The tiled records, [(frame indices, merged records)] of the B frames of one source.  Every window
        (ops.tile_windows) is a crop view of the frames on the device, read in place by its input launch.  Windows of one
        network input size are one [n*B,3,Hp,Wp] batch, window-major, built in place; the full-frame window joins the tiles'
        batch when its input size equals theirs and is a second batch otherwise.  Forward and post-process are self._records
        (graph capture by shape as everywhere), then the boxes go back to window pixels and ONE merge launch pair makes the B
        frame records.  With an Nms the windows run the whole mode; the merge stays a hard NMS and takes the mode's `agnostic`."""
        tiles, B = call.tiles, src.n
        windows = ops.tile_windows(src.hw[0], src.hw[1], tiles.size, tiles.overlap, tiles.full_frame, src.align(tiles))
        dev = next(self.model.parameters()).device
        T = len(windows)
        by_input = {}
        for i, (_, _, h, w) in enumerate(windows):
            geo = self._geometry(h, w, call.preprocessing, call.input_size)
            by_input.setdefault(geo[2], []).append((i, geo))
        batches = []
        for (Hp, Wp), members in by_input.items():
            x = torch.empty((len(members) * B, 3, Hp, Wp), dtype=torch.float32, device=dev)
            for n, (i, geo) in enumerate(members):
                src.input(geo, out=x[n * B:(n + 1) * B], window=windows[i])
            # the views of ONE buffer (a graph replay hands out the fields as separate copies)
            rec = ops.record_views(self._records(x, call.conf_thres, call.nms_thres, call.rotated_nms, call.nms)['records'])
            pads = [geo[3] for _, geo in members for _ in range(B)]
            if any(p is not None for p in pads):
                ops.records_to_original_(rec, pads)
            batches.append(([i for i, _ in members], rec['records']))
        tile_records = batches[0][1]
        if len(batches) > 1:                                         # window order again: records only, 16 KiB each
            tile_records = tile_records.new_empty((T, B, tile_records.shape[1]))
            for idx, r in batches:
                tile_records[idx] = r.view(len(idx), B, -1)
        merged = ops.merge_tile_records(tile_records, B, T, [(x0, y0) for y0, x0, _, _ in windows],
                                        call.nms_thres if tiles.nms_thres is None else tiles.nms_thres, tiles.metric, call.rotated_nms,
                                        agnostic=call.nms is not None and call.nms.agnostic)
        merged['img_hw'] = [src.hw] * B
        return [(list(range(B)), merged)]

    def _records_of_views(self, src, call):
        """The augmented records, [(frame indices, fused records)] of the B frames of one source (one frame size).  Every view
        of call.augment is the frames mirrored and resized: its input is one launch over the frames in place
        (ops.frames_to_input / ops.yuv420_to_input with flip=).  The views of one network input size are one [n*B,3,Hp,Wp]
        batch, view-major, through self._records (graph capture by shape as everywhere); then the boxes go back to the pixels
        of the mirrored frame and ONE fusion launch pair (ops.fuse_view_records) makes the B frame records.  With an Nms every
        view runs the whole mode; the fusion takes the mode's `agnostic`."""
        aug, B = call.augment, src.n
        plan = aug.plan(call.input_size, self.divisibe, call.preprocessing)
        dev = next(self.model.parameters()).device
        V = len(plan)
        by_input, geos = {}, []
        for v, (size, flip) in enumerate(plan):
            geo = self._geometry(src.hw[0], src.hw[1], call.preprocessing, size)
            geos.append(geo)
            by_input.setdefault(geo[2], []).append((v, geo, flip))
        batches = []
        for (Hp, Wp), members in by_input.items():
            x = torch.empty((len(members) * B, 3, Hp, Wp), dtype=torch.float32, device=dev)
            for n, (_, geo, flip) in enumerate(members):
                src.input(geo, out=x[n * B:(n + 1) * B], flip=flip)
            # the views of ONE buffer (a graph replay hands out the fields as separate copies)
            rec = ops.record_views(self._records(x, call.conf_thres, call.nms_thres, call.rotated_nms, call.nms)['records'])
            pads = [geo[3] for _, geo, _ in members for _ in range(B)]
            if any(p is not None for p in pads):
                ops.records_to_original_(rec, pads)
            batches.append(([v for v, _, _ in members], rec['records']))
        view_records = batches[0][1]
        if len(batches) > 1:                                         # view order again: records only, 16 KiB each
            view_records = view_records.new_empty((V, B, view_records.shape[1]))
            for idx, r in batches:
                view_records[idx] = r.view(len(idx), B, -1)
        fused = ops.fuse_view_records(view_records, B, V, [flip for _, flip in plan], src.hw,
                                      call.nms_thres if aug.thres is None else aug.thres, aug.fuse, aug.metric,
                                      call.rotated_nms and aug.fuse == 'nms', call.nms is not None and call.nms.agnostic, aug.min_score)
        fused['img_hw'] = [src.hw if geos[0][3] is not None else geos[0][2]] * B
        return [(list(src.idxs), fused)]

    def _detect(self, make_sources, kwargs, draw=None, chips=None, redact=None):
        """The one path behind every frame method that returns objects.  make_sources(): the call's frame sources, built (and
        so checked) once the tracker's type is known to be right; draw: a Draw, or chips: a Chips, for the methods that go on
        to paint or cut out what was found (one source); redact: a Redact, for those that hide it in the frames, before anything
        is painted.  Returns the ImageObjects in frame order -- with draw or redact, (objects, what the source calls drawn); with
        chips, (objects, chip views).  An untracked call hands the records buffer to the
        draw or crop launch before any host synchronisation; a tracked call hands it to the tracker (_tracked_objects) and
        paints or cuts out the returned tracks."""
        tracker, coasting = self._pop_tracker(kwargs)
        zones = self._pop_zones(kwargs, tracker)
        overlay = self._pop_overlay(kwargs, tracker, zones, draw)
        motion = self._pop_companion(kwargs, 'motion', tracker)
        appearance = self._pop_appearance(kwargs, tracker)
        keyframes = self._pop_companion(kwargs, 'keyframes', tracker)
        sources = make_sources()
        used = draw is not None or chips is not None or redact is not None
        if tracker is not None:
            src = self._one_source(sources, 'tracked')
            tracker.check_call(src.n, src.hw, self.model.bb_format)
            for companion, args in ((zones, (src.hw, self.model.bb_format)), (overlay, (zones, src.hw)), (motion, (src.hw,)),
                                    (appearance, (src.hw,)), (keyframes, (src.hw,))):
                if companion is not None:
                    companion.check_call(tracker, *args)
        elif used:
            src, = sources                                           # a plain call alone takes any number of sizes, none included
        call = self._call_settings(kwargs, whole=tracker is not None or used)
        conf_thres = call.conf_thres
        if tracker is not None and tracker.low_thres is not None:
            # the second stage needs the low band in the records: every post-process of this call (the windows of tiles=
            # and the views of augment= included) runs at the lower threshold; the tracker keeps the call's own as high_thres
            tracker.assoc(conf_thres)
            call = self._call_settings(dict(kwargs, conf_thres=min(conf_thres, tracker.low_thres)), whole=True)
        if keyframes is None:
            records = self._source_records(sources, call)
        if tracker is not None:
            # the camera motion of the whole original frames (whatever tiles= and augment= fed the network), ahead of the tracker
            shift = None if motion is None else motion.run(*src.image(), tracker, src.hw)['shift']
            if keyframes is not None:                                # the network on the key frames, the carry on all of them
                records = self._carried_records(src, call, keyframes, tracker, shift)
            # the descriptors come from the whole original frames too, at the call's final records: behind the motion launches
            # (under the similarity model the tracker takes the model; the carry above keeps the centre's shift)
            found = objs = self._tracked_objects(records, src.hw, tracker, coasting, conf_thres, zones, overlay,
                                                 None if motion is None else motion.track_args(),
                                                 None if appearance is None else (appearance, src))
        elif used:
            records = list(records)
            (idxs, found), = records                                 # one frame size: one group, in frame order
            assert idxs == list(range(src.n))
        if redact is not None:
            made = src.redact(found, redact.style(src.hw))
        if overlay is not None:                                      # under the boxes and their labels, over the redaction
            overlay.paint(*src.image(), zones, src.hw, coasting)
        if draw is not None:
            made = src.draw(found, draw.style(src.hw, tracker is not None))
        elif chips is not None:
            made = src.crop(found, chips.kwargs(self.model.input_format))
        if tracker is None:                                          # after the launch: this is where the host waits for the counts
            objs = self._objects_of_records(records)
        if chips is not None:
            made = self._chip_views(made, objs)
        return (objs, made) if used else objs

    def predict_frames(self, frames, **kwargs):
        """predict_batch for decoded video: `frames` is a torch.uint8 tensor or numpy.uint8 array [B,H,W,3] (or [H,W,3]) in
        RGB order, on the host or already on the device, or a list of such frames (grouped by size).  No PIL object and no
        per-frame copy or launch: resize, padding, /255 and normalisation of a whole group are one HIP launch that gives
        the bits of preprocess_batch, so the detections equal predict_batch on PIL.Image.fromarray of the same frames.
        Keyword arguments as in _predict_pil (augment= included: an Augment runs mirrored and rescaled views of the frames,
        each read in place by its input launch, and fuses them on the device; frames of any sizes, not with tiles), and
        tiles: None, or a Tiles for tiled detection on large frames (frames of one size): every window's input is one launch over a crop view of all frames, the windows of one size are one forward
        batch, and one more NMS on the device merges their detections in frame coordinates (include/mydet.h:
        mydet_merge_tile_records_f32).  Returns a list of ImageObjects in original-frame coordinates.
        tracker: None, or a mydetection_amd.api.Tracker (frames of one size, a multiple of its `streams` of them: stream s owns
        the consecutive frames s*F .. s*F + F-1).  One more launch on the device (include/mydet.h: mydet_track_frames_f32)
        associates the call's detections with the tracker's tracks, and each ImageObjects then holds the tracks matched or born
        in its frame -- bboxes the Kalman-filtered state, scores the track scores, cats the classes, obj_ids (int64) the
        persistent identities -- and, with coasting=True, the live tracks without a detection in that frame as well.
        zones: None, or a mydetection_amd.api.Zones (with tracker= only: ValueError otherwise).  One more launch right behind the
        tracker's (include/mydet.h: mydet_zones_frames) counts the tracks in its polygons and across its lines; the objects are
        bit for bit those of the call without zones= and carry zone_mask (int32: bit z = inside polygon z) and line_events
        (int32: bit 2l / 2l+1 = went through line l in its positive / negative direction in this frame); zones.last,
        zones.counts() and zones.heat have the rest.  Every frame method that takes tracker= takes zones=.
        motion: None, or a mydetection_amd.api.CameraMotion (with tracker= only: ValueError otherwise) for a camera that moves.
        Its launches run on the call's whole original frames before the tracker's (include/mydet.h: mydet_motion_frames_rgb_u8),
        give one integer shift (dx, dy) per frame against the frame before it, and the tracker moves every prediction by it
        before the association (mydet_track_frames_motion_f32); no host synchronisation is added, motion.last has the shifts.
        A CameraMotion(model='similarity') fits shift, rotation and zoom (mydet_motion_warp_frames_rgb_u8): the tracker's launch
        then takes motion.last['warp'] and moves, turns and scales every prediction (mydet_track_frames_warp_f32), while the
        key-frame carry keeps reading motion.last['shift'], the motion of the frame centre.
        Zones, trails and the heat map stay in frame pixels and assume a fixed camera.  Every frame method that takes tracker=
        takes motion=; without it every call is bit for bit what it was.
        appearance: None, or a mydetection_amd.api.Appearance (with tracker= only, and only with its assign='greedy': ValueError
        otherwise) to match by what an object looks like too.  One launch on the call's whole original frames and its final
        records (after the tile merge or the view fusion, behind the motion launches; include/mydet.h:
        mydet_appear_boxes_rgb_u8) gives every detection a 128-bin colour descriptor -- 32 x 16 nearest-pixel samples over the
        central 0.75 of the box, a 4 x 4 x 4 colour histogram for its upper and one for its lower half --, and the tracker launch
        (mydet_track_frames_appear_f32) keeps a template per track, offers an IoU match only when the histogram intersection
        reaches `gate`, and gives a detection that would start a track to the most similar lost track within `reach` instead
        when it reaches `reid`.  An Appearance(weight=...) runs with a tracker of assign='optimal' instead (a greedy one is the
        ValueError then): each stage is one minimum-cost assignment on a fused IoU-and-similarity cost
        (mydet_track_frames_appear_optimal_f32), the gate and the re-identification as before.
        No host synchronisation is added; appearance.last has desc, sim and how.  Every frame method
        that takes tracker= takes appearance=; without it every call is bit for bit what it was.
        keyframes: None, or a mydetection_amd.api.KeyFrames (with tracker= only: ValueError otherwise) to run the network on every
        n-th frame of a stream only.  Its counter says which frames of the call are key frames (host arithmetic, calls of any
        length continue each other); only those go through the input launch, the forward pass and the post-process (tiles= and
        augment= included), as a strided view or one gather of the frames.  One launch pair on the call's whole original frames
        (include/mydet.h: mydet_carry_records_rgb_u8) then makes the record of every frame: a key frame's is the detector's,
        an in-between frame's holds the key boxes moved to where their pixels are found -- block matching against a template
        taken at the key frame, around the box's last step and the camera's shift (motion=) --, and a box whose pixels are
        flat, gone or out of the frame is left out, so that its track coasts as on any miss.  The tracker, the zones, the
        trails and everything that paints read those records as any others; no host synchronisation is added; keyframes.last has
        how, offset and sad.  every=1 gives the objects of the call without keyframes=, bit for bit.  Every frame method that
        takes tracker= takes keyframes=; without it every call is bit for bit what it was."""
        return self._detect(lambda: self._rgb_sources(frames), kwargs)

    @staticmethod
    def _pop_tracker(kwargs):
        """(tracker, coasting) out of a frame method's keyword arguments; a TypeError for anything but a Tracker."""
        from .tracking import Tracker
        tracker, coasting = kwargs.pop('tracker', None), bool(kwargs.pop('coasting', False))
        if tracker is not None and not isinstance(tracker, Tracker):
            raise TypeError(f'tracker: a mydetection_amd.api.Tracker (or None) expected, got {type(tracker).__name__}')
        return tracker, coasting

    # the objects that sit behind the tracker in a tracked call: keyword -> (class, why it needs a tracker; None for the overlay,
    # whose check_call has that rule, behind the TypeError of a method that does not draw)
    _COMPANIONS = {'zones': (Zones, 'zones= counts tracks'),
                   'overlay': (Overlay, None),
                   'motion': (CameraMotion, 'motion= moves the predictions of a tracker'),
                   'appearance': (Appearance, 'appearance= gates and re-identifies the tracks of a tracker'),
                   'keyframes': (KeyFrames, 'keyframes= fills the frames between key frames for a tracker')}

    @staticmethod
    def _pop_companion(kwargs, key, tracker):
        """The `key` entry out of a frame method's keyword arguments: a TypeError for anything but None or an object of its
        class, a ValueError without a tracker, both before any launch."""
        cls, why = Detector._COMPANIONS[key]
        obj = kwargs.pop(key, None)
        if obj is not None and not isinstance(obj, cls):
            raise TypeError(f'{key}: a mydetection_amd.api.{cls.__name__} (or None) expected, got {type(obj).__name__}')
        if obj is not None and tracker is None and why:
            raise ValueError(f'{key}: {why} and needs tracker= in the same call')
        return obj

    @staticmethod
    def _pop_zones(kwargs, tracker):
        """zones out of a frame method's keyword arguments, by _pop_companion's rules."""
        return Detector._pop_companion(kwargs, 'zones', tracker)

    @staticmethod
    def _pop_appearance(kwargs, tracker):
        """As _pop_companion, and a ValueError with a tracker whose assignment is not the one the object runs with: 'greedy'
        without a weight, 'optimal' with one."""
        appearance = Detector._pop_companion(kwargs, 'appearance', tracker)
        if appearance is not None:
            appearance.check_tracker(tracker)
        return appearance

    @staticmethod
    def _pop_overlay(kwargs, tracker, zones, draw):
        """As _pop_companion, and a TypeError in a method that does not draw, a ValueError for the zone parts without zones=."""
        overlay = Detector._pop_companion(kwargs, 'overlay', tracker)
        if overlay is not None:
            if draw is None:
                raise TypeError('overlay: overlay= is an argument of annotate_frames and its YUV forms')
            overlay.check_call(tracker, zones, (1, 1) if overlay.img_hw is None else overlay.img_hw)
        return overlay

    @staticmethod
    def _no_tracker(kwargs, what):
        if 'tracker' in kwargs or 'coasting' in kwargs or 'zones' in kwargs or 'motion' in kwargs or 'appearance' in kwargs or 'keyframes' in kwargs:
            raise TypeError(f'{what}: track ids in the json rows are not built; use the predict_frames form with tracker=')

    def _tracked_objects(self, records, frame_hw, tracker, coasting, conf_thres, zones=None, overlay=None, camera=None, appearance=None):
        """The tracked form of _objects_of_records: one eager tracker launch on the call's records (frame coordinates, one
        buffer), then per frame the ImageObjects of the tracks with missed == 0 (coasting: of every live track).  Two host
        synchronisations: the frame counts, and the indices of the selected slots.  zones: a Zones whose launch follows the
        tracker's at once (no synchronisation in between); the objects then carry zone_mask and line_events.  overlay: an
        Overlay, whose trails launch follows them and which keeps the tracker's outputs for its paint launch.  camera: the
        camera motion of the call's frames (CameraMotion.track_args: shift= or warp=), on the device.  appearance: (an Appearance, the call's frame
        source): its descriptor launch on these records runs right ahead of the tracker's."""
        from ..utils.structures import ImageObjects
        records = list(records)
        assert len(records) == 1, 'one frame size gives one network input size'
        idxs, rec = records[0]
        assert idxs == list(range(len(idxs)))
        hw = rec['img_hw'][0]                                        # what the untracked call reports
        width = 5 if 'angle' in rec else 4
        state = tracker.bind(frame_hw, width, rec['records'].device)
        params = tracker.params(frame_hw, tracker.resolve_match(self.model.bb_format), conf_thres)
        assoc, appear, fused = tracker.assoc(conf_thres), None, {}
        if appearance is not None:
            birth = max(params.new_thres, assoc.high_thres) if assoc is not None and assoc.bands else params.new_thres
            appear = appearance[0].run(*appearance[1].image(), rec, tracker, frame_hw, birth)
            fused = appearance[0].launch_args()
        out = ops.track_frames(rec, state, params, max_tracks=tracker.max_tracks, assoc=assoc, appear=appear, **(camera or {}), **fused)
        if appearance is not None:
            appearance[0].took(out)
        zout = None if zones is None else zones.run(out, tracker, frame_hw)
        if overlay is not None:                                      # the trails launch, behind the tracker's (and the zones')
            overlay.run_trails(out, tracker, zones, frame_hw)
        B, mt = len(idxs), tracker.max_tracks
        missed = out['missed'].view(B, mt)
        keep = (missed >= 0) if coasting else (missed == 0)
        ops.check_counts(out['count'].view(B).cpu().tolist())
        sel = keep.nonzero()
        per_frame = torch.bincount(sel[:, 0], minlength=B).cpu().tolist()
        box, score, cls, ids = out['box'].view(B * mt, 5), out['score'].view(-1), out['cls'].view(-1), out['id'].view(-1)
        flat = sel[:, 0] * mt + sel[:, 1]
        inside, crossed = (None, None) if zout is None else (zout['inside'].view(-1), zout['crossed'].view(-1))
        objs, lo = [], 0
        for k in per_frame:
            rows = flat[lo:lo + k]
            lo += k
            objs.append(ImageObjects(box[rows][:, :width], cls[rows], None, score[rows], self.model.bb_format, hw, obj_ids=ids[rows],
                                     zone_mask=None if inside is None else inside[rows],
                                     line_events=None if crossed is None else crossed[rows]))
        return objs

    def _objects_of_records(self, records):
        """ImageObjects in frame order from the (indices, records) pairs of _records_of_inputs."""
        from ..parallel import records_to_objects
        out = []
        for idxs, rec in records:
            out += [None] * (max(idxs) + 1 - len(out))
            objs = records_to_objects(rec, bb_format=self.model.bb_format)
            for j, o, hw in zip(idxs, objs, rec['img_hw']):
                o.img_hw = hw
                out[j] = o
        return out

    def frames_to_json(self, frames, img_ids, eval_type='x1y1wh', catIdx2id=None, **kwargs):
        """COCO-style rows of uint8 frames (see predict_frames), image by image: the counterpart of _json_batch."""
        self._no_tracker(kwargs, 'frames_to_json')
        return self._json_of_records(self._frame_records(frames, **kwargs), img_ids, eval_type, catIdx2id)

    def _json_of_records(self, records, img_ids, eval_type, catIdx2id):
        """COCO-style rows in frame order from the (indices, records) pairs of _records_of_inputs."""
        from ..utils.structures import batched_to_json
        out = [None] * len(img_ids)
        for idxs, rec in records:
            rows = batched_to_json(rec, [img_ids[j] for j in idxs], eval_type, catIdx2id)
            counts = ops.check_counts(rec['count'].cpu().tolist())
            o = 0
            for j, k in zip(idxs, counts):
                out[j] = rows[o:o + k]
                o += k
        return [d for per_img in out for d in per_img]

    @staticmethod
    def _yuv_planes(planes, layout, device=None):
        """4:2:0 frames of `layout` (ops.YUV420_LAYOUTS) as the tensors ops.yuv420_to_input takes: [y [B,H,W], uv
        [B,ceil(H/2),ceil(W/2),2]] or [y, u, v] with chroma planes [B,ceil(H/2),ceil(W/2)] ('yv12': y, v, u).  planes: a tuple
        of torch tensors or numpy arrays (2-d planes mean one frame) -- uint8 for the 8-bit layouts, numpy.uint16 / torch.int16
        / torch.uint16 words for 'p010' and 'i010' -- or ONE array: a decoder's contiguous surface [B,H*3/2,W] (or 2-d) with
        even H and W, Y then the chroma plane(s) in storage order, split into views that share its storage.  Anything else is
        a ValueError (layout name, shape) or a TypeError (type, dtype).  device: where the data goes before the split -- one
        copy per plane or surface, none for what is already there; None leaves it where it is, and then no device is touched."""
        _, bps, planar = ops.yuv420_layout(layout)
        what = 'predict_frames_yuv'
        np_dtype = np.uint8 if bps == 1 else np.uint16

        def tensor(f):                                               # a numpy array as a tensor; ops has the rules for tensors
            if not isinstance(f, np.ndarray):
                return f
            if f.dtype != np_dtype:
                raise TypeError(f'{what}: {layout!r} planes are numpy arrays of dtype {np.dtype(np_dtype)}, got {f.dtype}')
            f = np.ascontiguousarray(f)
            return torch.from_numpy(f if bps == 1 else f.view(np.int16))            # the same bits

        if isinstance(planes, (np.ndarray, torch.Tensor)):
            s = ops.yuv420_samples(tensor(planes), layout, what)
            if s.dim() not in (2, 3) or min(s.shape) < 1:
                raise ValueError(f'{what}: a surface of shape [B,H*3/2,W] or [H*3/2,W] expected, got {tuple(s.shape)}')
            rows, W = s.shape[-2:]
            H = rows // 3 * 2
            if rows % 3 or W % 2:                                    # an odd H would give 3k + 2 rows
                raise ValueError(f'{what}: a single {layout!r} surface has H*3/2 rows with even H and W, got {tuple(s.shape)}')
            s = s if device is None else s.to(device, non_blocking=True)
            s = s.unsqueeze(0) if s.dim() == 2 else s
            if not planar:
                return [s[:, :H], s[:, H:].unflatten(2, (W // 2, 2))]
            if not s[0].is_contiguous():
                s = s.contiguous()
            chroma = s[:, H:].flatten(1)                             # a view: the rows of a frame are packed
            n = (H // 2) * (W // 2)
            return [s[:, :H], chroma[:, :n].unflatten(1, (H // 2, W // 2)), chroma[:, n:].unflatten(1, (H // 2, W // 2))]
        if not isinstance(planes, (tuple, list)):
            raise TypeError(f'{what}: a tuple of planes or one surface array expected, got {type(planes).__name__}')
        ts, _ = ops.yuv420_check_planes([tensor(f) for f in planes], layout, what)
        if device is not None:
            ts = [t.to(device, non_blocking=True) for t in ts]
        return ts

    def predict_frames_yuv(self, planes, layout, *, matrix='bt601', full_range=False, **kwargs):
        """predict_frames for 4:2:0 video in any layout decoders give: 'nv12', 'nv21' (8-bit, interleaved chroma), 'i420',
        'yv12' (8-bit, planar), 'p010' (10 bits in the high end of 16-bit words, interleaved) and 'i010' (yuv420p10le: 10
        bits in the low end, planar).  planes: (y, uv) or (y, u, v) ('yv12': (y, v, u)) as torch tensors or numpy arrays, or a
        single decoder surface [B,H*3/2,W] with even H and W (see _yuv_planes); host data crosses in one copy per plane or
        surface, device tensors are read in place through their strides.  A 10-bit sample becomes 8 bits by
        min(255, (v + 2) >> 2); from there the conversion is NV12's (include/mydet.h).  Returns exactly what
        predict_frames returns for the converted RGB frames (ops.yuv420_to_rgb), which are never built: one HIP launch
        reads the planes.  One call takes one frame size.  Keyword arguments as in _predict_pil and predict_frames (tiles:
        even frame and tile sizes; tracker, coasting)."""
        return self._detect(lambda: [_Yuv420Frames(self, planes, layout, matrix, full_range)], kwargs)

    def frames_yuv_to_json(self, planes, layout, img_ids, eval_type='x1y1wh', catIdx2id=None, *, matrix='bt601', full_range=False,
                           **kwargs):
        """COCO-style rows of 4:2:0 frames (see predict_frames_yuv): the counterpart of frames_to_json."""
        self._no_tracker(kwargs, 'frames_yuv_to_json')
        records = self._source_records([_Yuv420Frames(self, planes, layout, matrix, full_range)], self._call_settings(kwargs))
        return self._json_of_records(records, img_ids, eval_type, catIdx2id)

    def predict_frames_nv12(self, y, uv=None, *, matrix='bt601', full_range=False, **kwargs):
        """predict_frames for NV12 video, the format decoders produce: y is the uint8 Y plane [B,H,W] (or [H,W]) and uv the
        interleaved chroma plane [B,ceil(H/2),ceil(W/2),2]; or, with uv=None, y is the single surface [B,H*3/2,W] (or 2-d)
        with even H and W, split into the two plane views without a copy.  torch tensors or numpy arrays; host data
        crosses in one copy per plane or surface, device tensors are read in place through their strides.  matrix:
        'bt601' or 'bt709'; full_range: Y in 0..255 instead of 16..235 (formula: include/mydet.h).  Returns
        exactly what predict_frames returns for the converted RGB frames (ops.nv12_to_rgb), which are never built: one
        HIP launch reads the planes.  One call takes one frame size.  Keyword arguments as in _predict_pil."""
        return self.predict_frames_yuv(y if uv is None else (y, uv), 'nv12', matrix=matrix, full_range=full_range, **kwargs)

    def frames_nv12_to_json(self, y, uv, img_ids, eval_type='x1y1wh', catIdx2id=None, *, matrix='bt601', full_range=False, **kwargs):
        """COCO-style rows of NV12 frames (see predict_frames_nv12): the counterpart of frames_to_json."""
        return self.frames_yuv_to_json(y if uv is None else (y, uv), 'nv12', img_ids, eval_type, catIdx2id, matrix=matrix,
                                       full_range=full_range, **kwargs)

    @staticmethod
    def _setting(given, kind, what):
        """The Draw or Chips (`kind`) of a call: the default one for None, a TypeError for anything else."""
        if given is not None and not isinstance(given, kind):
            raise TypeError(f'{what}: {kind.__name__.lower()} is a mydetection_amd.api.{kind.__name__}, got {type(given).__name__}')
        return kind() if given is None else given

    def annotate_frames(self, frames, draw=None, redact=None, **kwargs):
        """predict_frames plus the overlay: returns (objects, drawn).  objects is exactly what predict_frames(frames, **kwargs)
        returns; drawn is the uint8 batch [B,H,W,3] on the device with boxes, fills and labels painted by ONE more launch
        (include/mydet.h: mydet_draw_boxes_rgb_u8) -- the input itself, drawn in place, when it is a single device tensor with
        packed pixels, else the device batch the call had to build anyway.  Frames of one size (ValueError otherwise).  draw: a
        Draw (default Draw()).  tiles=, tracker= and coasting= as in predict_frames.  An untracked call draws straight from the
        records buffer, before any host synchronisation; a tracked call draws the returned tracks, with their ids.  redact: None,
        or a Redact: the detections are hidden first (as redact_frames does) and the overlay is painted on top.
        overlay: None, or a mydetection_amd.api.Overlay (with tracker=; its zone parts with zones=: ValueError otherwise): the
        zones and lines of the call's Zones, their counters as they stand after each frame and the trails of the tracks are
        painted by one more launch before the boxes (include/mydet.h: mydet_draw_overlay_rgb_u8), the trails kept by one launch
        behind the tracker's (mydet_trails_frames); no host synchronisation is added and the objects are bit for bit those of
        the call without overlay=.  Paint order: redact, overlay, boxes.  annotate_frames_yuv and _nv12 take it too."""
        draw = self._setting(draw, Draw, 'annotate_frames')
        redact = self._redact_setting(redact, 'annotate_frames')
        return self._detect(lambda: self._rgb_sources(frames, 'annotate_frames'), kwargs, draw=draw, redact=redact)

    def annotate_frames_yuv(self, planes, layout, draw=None, redact=None, *, matrix='bt601', full_range=False, **kwargs):
        """predict_frames_yuv plus the overlay, painted into the planes (include/mydet.h: mydet_draw_boxes_yuv420_u8): returns
        (objects, drawn).  layout: 'nv12', 'nv21', 'i420' or 'yv12'; the 10-bit layouts are not drawn into (ValueError).  drawn:
        the planes on the device, in the order given -- the input tensors themselves when they are device tensors -- or, for a
        single surface, the surface.  matrix and full_range also say how the colours become Y'CbCr.  Otherwise as annotate_frames
        (redact= included)."""
        draw = self._setting(draw, Draw, 'annotate_frames_yuv')
        redact = self._redact_setting(redact, 'annotate_frames_yuv')
        return self._detect(lambda: [_Yuv420Frames(self, planes, layout, matrix, full_range, drawn_by='annotate_frames_yuv')], kwargs,
                            draw=draw, redact=redact)

    def annotate_frames_nv12(self, y, uv=None, draw=None, redact=None, *, matrix='bt601', full_range=False, **kwargs):
        """annotate_frames_yuv for NV12: (y, uv) planes, or with uv=None the single surface [B,H*3/2,W] (see predict_frames_nv12)."""
        return self.annotate_frames_yuv(y if uv is None else (y, uv), 'nv12', draw, redact, matrix=matrix, full_range=full_range, **kwargs)

    @staticmethod
    def _redact_setting(given, what):
        """The `redact=` of an annotate_frames* call: None, or a Redact (a TypeError for anything else)."""
        if given is not None and not isinstance(given, Redact):
            raise TypeError(f'{what}: redact is a mydetection_amd.api.Redact (or None), got {type(given).__name__}')
        return given

    def redact_frames(self, frames, redact=None, **kwargs):
        """predict_frames plus the privacy step: returns (objects, redacted).  objects is exactly what predict_frames(frames,
        **kwargs) returns (tiles=, augment=, nms=, tracker=, coasting= and zones= included); redacted is the uint8 batch
        [B,H,W,3] on the device in which every detection is pixelated, blurred or painted over (include/mydet.h:
        mydet_redact_boxes_rgb_u8) -- the input itself, redacted in place, when it is a single device tensor with packed
        pixels, else the device batch the call had to build anyway.  Frames of one size (ValueError otherwise).  redact: a
        Redact (default Redact(): a mosaic of every detection).  An untracked call launches straight from the records buffer,
        before any host synchronisation.  A tracked call redacts the returned tracks: with coasting=True a person stays hidden
        through the frames in which the detector misses them, as long as the track lives."""
        redact = self._setting(redact, Redact, 'redact_frames')
        return self._detect(lambda: self._rgb_sources(frames, 'redact_frames'), kwargs, redact=redact)

    def redact_frames_yuv(self, planes, layout, redact=None, *, matrix='bt601', full_range=False, **kwargs):
        """predict_frames_yuv plus the privacy step, in the planes (include/mydet.h: mydet_redact_boxes_yuv420_u8): returns
        (objects, redacted).  layout: 'nv12', 'nv21', 'i420' or 'yv12'; the 10-bit layouts are not written into (ValueError).
        redacted: the planes on the device, in the order given -- the input tensors themselves when they are device tensors -- or,
        for a single surface, the surface.  matrix and full_range also say how the colour of 'solid' becomes Y'CbCr.  Otherwise
        as redact_frames."""
        redact = self._setting(redact, Redact, 'redact_frames_yuv')
        return self._detect(lambda: [_Yuv420Frames(self, planes, layout, matrix, full_range, drawn_by='redact_frames_yuv')], kwargs,
                            redact=redact)

    def redact_frames_nv12(self, y, uv=None, redact=None, *, matrix='bt601', full_range=False, **kwargs):
        """redact_frames_yuv for NV12: (y, uv) planes, or with uv=None the single surface [B,H*3/2,W] (see predict_frames_nv12)."""
        return self.redact_frames_yuv(y if uv is None else (y, uv), 'nv12', redact, matrix=matrix, full_range=full_range, **kwargs)

    @staticmethod
    def _chip_views(buf, objs):
        """One view per frame of the chip buffer [B,M,...]: the chips of the frame's first min(len(objects), M) rows."""
        return [buf[b, :min(len(o), buf.shape[1])] for b, o in enumerate(objs)]

    def crop_frames(self, frames, chips=None, **kwargs):
        """predict_frames plus the object chips: returns (objects, chips).  objects is exactly what predict_frames(frames,
        **kwargs) returns; chips is a list with one entry per frame, entry b a view [n_b,3,h,w] float32 (Chips(out='uint8'):
        [n_b,h,w,3] uint8) of ONE device buffer written by ONE more launch (include/mydet.h: mydet_crop_boxes_rgb): chip k of
        frame b shows row k of objects[b] -- its box scaled by `pad`, cut out of the frame, turned upright when the model
        predicts rotated boxes, resampled to `size`.  A frame with more objects than chips.max_per_frame gets chips for its
        first max_per_frame rows only (n_b = min(len(objects[b]), max_per_frame)).  Frames of one size (ValueError otherwise).
        chips: a Chips (default Chips()).  tiles=, tracker= and coasting= as in predict_frames.  An untracked call launches
        straight from the records buffer, before any host synchronisation; a tracked call crops the tracks' filtered boxes."""
        chips = self._setting(chips, Chips, 'crop_frames')
        return self._detect(lambda: self._rgb_sources(frames, 'crop_frames'), kwargs, chips=chips)

    def crop_frames_yuv(self, planes, layout, chips=None, *, matrix='bt601', full_range=False, **kwargs):
        """predict_frames_yuv plus the object chips, cut straight out of the planes (include/mydet.h: mydet_crop_boxes_yuv420):
        returns (objects, chips) as crop_frames does, the chips being those of the converted RGB frames (ops.yuv420_to_rgb),
        which are never built.  Every layout of predict_frames_yuv is accepted, the 10-bit ones included: crops only read."""
        chips = self._setting(chips, Chips, 'crop_frames_yuv')
        return self._detect(lambda: [_Yuv420Frames(self, planes, layout, matrix, full_range)], kwargs, chips=chips)

    def crop_frames_nv12(self, y, uv=None, chips=None, *, matrix='bt601', full_range=False, **kwargs):
        """crop_frames_yuv for NV12: (y, uv) planes, or with uv=None the single surface [B,H*3/2,W] (see predict_frames_nv12)."""
        return self.crop_frames_yuv(y if uv is None else (y, uv), 'nv12', chips, matrix=matrix, full_range=full_range, **kwargs)

    def predict_batch(self, pil_imgs, **kwargs):
        """Batched form of detect_one (the reference loops image by image, api/detection.py:67-74): images that share a
        network input size go through ONE forward + ONE batched post-process.  Returns a list of ImageObjects in the
        original image coordinates, in input order."""
        return self._objects_of_records(self._records_by_size(pil_imgs, **kwargs))
