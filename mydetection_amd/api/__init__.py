"""Inference entry point of the package: `Detector` (mirror of the reference's api.detection.Detector), `Tiles`, the
argument of its tiled detection on large frames, and `Tracker`, the argument that turns its frame methods into a tracker."""
from .detection import Detector, Tiles
from .tracking import Tracker

__all__ = ['Detector', 'Tiles', 'Tracker']
