"""Error-bounded variable-width compression: the reference has it for TensorFlow only, so the codec of
grace_amd/inceptionn.py is the implementation."""
from grace_amd.inceptionn import InceptionnCompressor

__all__ = ["InceptionnCompressor"]
