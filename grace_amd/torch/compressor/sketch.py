"""Quantile-bucket quantisation: the reference has it for TensorFlow only, so the codec of
grace_amd/sketch.py is the implementation."""
from grace_amd.sketch import SketchCompressor

__all__ = ["SketchCompressor"]
