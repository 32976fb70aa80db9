"""Inference entry point of the package: `Detector` (mirror of the reference's api.detection.Detector) and `Tiles`, the
argument of its tiled detection on large frames."""
from .detection import Detector, Tiles

__all__ = ['Detector', 'Tiles']
