"""Inference entry point of the package: `Detector` (mirror of the reference's api.detection.Detector), `Tiles`, the
argument of its tiled detection on large frames, `Tracker`, the argument that turns its frame methods into a tracker,
`Draw`, the settings of its annotate_frames methods, and `Chips`, the settings of its crop_frames methods."""
from .detection import Chips, Detector, Draw, Tiles
from .tracking import Tracker

__all__ = ['Chips', 'Detector', 'Draw', 'Tiles', 'Tracker']
