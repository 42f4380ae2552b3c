"""8-bit codebook quantisation: the reference has it for TensorFlow only, so the codec of
grace_amd/u8bit.py is the implementation."""
from grace_amd.u8bit import U8bitCompressor

__all__ = ["U8bitCompressor"]
