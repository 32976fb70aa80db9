"""Inference entry point of the package: `Detector` (mirror of the reference's api.detection.Detector), `Tiles`, the
argument of its tiled detection on large frames, `Tracker`, the argument that turns its frame methods into a tracker,
`Draw`, the settings of its annotate_frames methods, `Redact`, the settings of its redact_frames methods (mosaic, blur or one
colour over every detection, on the device), `Chips`, the settings of its crop_frames methods, `Nms`, how its
post-process suppresses (class-agnostic, Soft-NMS, box merging), `Augment`, its test-time augmentation (mirrored and rescaled
views fused on the device), `Evaluator`, which scores what it returns against ground
truth, `TrackEvaluator`, which scores its tracks against ground-truth identities, `Zones`, which counts its tracks in
polygons and across lines on the device, and `Overlay`, which paints those zones, lines, counters and the tracks' trails into
the annotated frames, and `CameraMotion`, which estimates the global image shift of every frame on the device and moves the
tracker's predictions by it, and `Appearance`, which gives every detection a colour descriptor on the device and lets the
tracker gate its matches and re-identify lost tracks by it, and `KeyFrames`, which runs the network on every n-th frame only and
carries the boxes through the frames between by their pixels, on the device."""
from .appearance import Appearance
from .detection import Augment, Chips, Detector, Draw, Nms, Redact, Tiles
from .evaluation import Evaluator, TrackEvaluator
from .keyframes import KeyFrames
from .motion import CameraMotion
from .overlay import Overlay
from .tracking import Tracker
from .zones import Zones

__all__ = ['Appearance', 'Augment', 'CameraMotion', 'Chips', 'Detector', 'Draw', 'Evaluator', 'KeyFrames', 'Nms', 'Overlay', 'Redact', 'Tiles', 'TrackEvaluator', 'Tracker', 'Zones']
