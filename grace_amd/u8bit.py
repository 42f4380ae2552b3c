"""8-bit codebook quantisation (Dettmers, arXiv:1511.04561; grace_dl/tensorflow/compressor/u8bit.py):
int8 codes into a non-uniform table of 128 magnitudes, scaled by the absolute maximum of the tensor
(``block_size=0``, the reference's single scaler) or of each block of 256 to 4096 elements.
Deterministic, stateless, fixed rate: n bytes of codes and 4 bytes a block on the wire, the same for a
float32 and a bfloat16 gradient.  The arithmetic is stated in include/grace_hip_u8bit.h.

Two deliberate departures from the reference file: it leaves a ratio |x| / max below its first edge and
above its last edge -- where the maximum itself falls -- to a NaN -> int8 cast; here those clamp to
codes 0 and 127.  The default table is built from the published dynamic-tree construction
(``ops.u8bit_host_tables``), not copied; ``rounding="floor"`` decodes to the lower edge as the
reference does, ``"nearest"`` to the nearer value, and ``codebook`` takes 128 ascending values.

``Allgather(U8bitCompressor(...), NoneMemory(), W).step`` on a CUDA float32 or bfloat16 tensor is
fused at every world size (one launch at world 1 block-wise, two tensor-wide; the codes never reach
memory) and returns the gradient's dtype.  ``compress`` / ``decompress`` by hand, and so
ResidualMemory, take float32; bfloat16 there and float16 anywhere raise TypeError.  AllToAll is not
served.  Blocks are counted from element 0 of the tensor handed in, so a step over a flat bucket needs
no segment table: blocks may span the tensors in it.

The codec lives beside the other codecs added after the first release (``grace_amd/cast_bf16.py``,
``quant_bf16.py``, ...): import ``U8bitCompressor`` and ``grace_from_params`` from here.
``grace_from_params`` below is grace_amd.dist's with the key ``'u8bit'`` (and its optional
``block_size`` and ``rounding``) added; every other params dict is handed to grace_amd.dist's
unchanged, which itself keeps raising NotImplementedError for ``'u8bit'``.
"""
import torch

from grace_amd import ops
from grace_amd.dist import Compressor
from grace_amd.dist.communicator.allgather import Allgather, _gather_flat
from grace_amd.dist.memory.none import NoneMemory


class U8bitCompressor(Compressor):

    def __init__(self, block_size=0, rounding="floor", codebook=None):
        super().__init__(tensors_size_are_same=True)
        self.block_size = ops._u8bit_block(block_size, "U8bitCompressor")
        values = ops.u8bit_host_tables(rounding, codebook)[1]   # validated here, on the host; ValueError
        self.rounding = rounding
        self.codebook = None if codebook is None else tuple(values.tolist())
        self._dev = {}

    def _tables(self):
        """(edges, values) on the current device, looked up once per device"""
        d = torch.cuda.current_device()
        tabs = self._dev.get(d)
        if tabs is None:
            tabs = self._dev[d] = ops.u8bit_tables(self.rounding, self.codebook)
        return tabs

    def compress(self, tensor, name):
        flat = ops.dev_f32(tensor)
        codes, scales = ops.u8bit_compress(flat, self.block_size, self._tables()[0])
        return [codes, scales], (tensor.dtype, tensor.size())

    def decompress(self, tensor_compressed, ctx):
        codes, scales = tensor_compressed
        dtype, shape = ctx
        return ops.u8bit_decode_aggregate(codes, scales, 1, shape.numel(), self.block_size, self._tables()[1],
                                          out_dtype=dtype).view(shape)

    def decode_aggregate_gathered(self, gathered, ctx, world_size):
        codes, scales = gathered
        if not codes.is_cuda:
            return None
        dtype, shape = ctx
        return ops.u8bit_decode_aggregate(codes, scales, world_size, shape.numel(), self.block_size,
                                          self._tables()[1], divisor=world_size if self.average else 1.0,
                                          out_dtype=dtype).view(shape)

    def fused_step(self, communicator, tensor, name):
        if not (communicator.__class__ is Allgather and communicator.memory.__class__ is NoneMemory
                and isinstance(tensor, torch.Tensor) and tensor.is_cuda and tensor.dtype in (ops.F32, ops.BF16)):
            return None
        edges, values = self._tables()
        world = int(communicator.world_size)
        if world == 1:
            return ops.u8bit_step_w1(tensor, self.block_size, edges, values)[1]
        g = ops.dev_grad(tensor)
        codes, scales = ops.u8bit_compress(g, self.block_size, edges)
        codes, scales = _gather_flat(codes, world), _gather_flat(scales, world)
        return ops.u8bit_decode_aggregate(codes, scales, world, g.numel(), self.block_size, values,
                                          divisor=world if self.average else 1.0,
                                          out_dtype=g.dtype).view(tensor.shape)


def grace_from_params(params):
    """grace_amd.dist.helper.grace_from_params, plus ``'compressor': 'u8bit'`` with the optional keys
    ``block_size`` (0) and ``rounding`` ('floor'); memory and communicator as there."""
    from grace_amd.dist.helper import grace_from_params as dist_from_params
    if params.get('compressor', 'none') != 'u8bit':
        return dist_from_params(params)
    compressor = U8bitCompressor(params.get('block_size', 0), params.get('rounding', 'floor'))
    comm = dist_from_params({**params, 'compressor': 'none'})   # the memory and the communicator
    comm.compressor = compressor
    return comm
