"""Microscaling (block-scaled FP8, FP6 and FP4): the reference has no such codec, so the one of
grace_amd/mx.py is the implementation."""
from grace_amd.mx import MXCompressor

__all__ = ["MXCompressor"]
