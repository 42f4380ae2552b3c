"""Adaptive quantisation: the reference has it for TensorFlow only, so the codec of grace_amd/adaq.py is the
implementation."""
from grace_amd.adaq import AdaqCompressor

__all__ = ["AdaqCompressor"]
