"""Adaptive quantisation (AdaQ: Dryden, Moon, Jacobs and Van Essen, MLHPC 2016;
grace_dl/tensorflow/compressor/adaq.py): the ``compress_ratio`` largest positive elements travel as one
mean, the same share of the negative ones as another, and a selected element sends only its position
and its sign: 2 bytes an entry (top-k's grouped payload costs 6, plain {value, index} 8, the reference's
adaq 4).  Stateless; the wire is the same for a float32 and a bfloat16 gradient.  The arithmetic and the
wire are stated in include/grace_hip_adaq.h.  The method drops most of the gradient's mass, so it is
meant to run with error feedback (``ResidualMemory``).

Deliberate departures from the reference file.  It finds its two thresholds from a 1 % sample and a
20-step correction loop, which leaves the count anywhere in 0.8 to 1.25 times the target and the wire at a
variable size; here each class's k = ceil(m * ratio) largest are selected exactly, ties to the lower
index.  The payload's size is then known on the host from (n, ratio), and the exchange is one
``all_gather_into_tensor`` with no size exchange and no host read.  It sends 32-bit indices; here an
entry is an offset inside a chunk of 8192 elements behind a chunk directory.

``Allgather(AdaqCompressor(r), NoneMemory(), W).step`` on a CUDA float32 or bfloat16 tensor is fused at
every world size and returns the gradient's dtype.  ``compress`` / ``decompress`` by hand, and so
ResidualMemory, take float32; bfloat16 there and float16 anywhere raise TypeError.  Not served yet: a
fused ResidualMemory step, AllToAll, the sharded engines and the Horovod optimizer path.

``grace_from_params`` below is grace_amd.inceptionn's (and so grace_amd.dist's) with the key ``'adaq'``
and its ``compress_ratio`` (0.01) added; every other params dict is handed on unchanged.
"""
import torch

from grace_amd import ops
from grace_amd.dist import Compressor
from grace_amd.dist.communicator.allgather import Allgather, _gather_flat
from grace_amd.dist.memory.none import NoneMemory


class AdaqCompressor(Compressor):

    def __init__(self, compress_ratio=0.01):
        super().__init__(tensors_size_are_same=True)
        self.compress_ratio = ops._adaq_ratio(compress_ratio, "AdaqCompressor")

    def compress(self, tensor, name):
        return [ops.adaq_compress(ops.dev_f32(tensor), self.compress_ratio)], (tensor.dtype, tensor.size())

    def decompress(self, tensor_compressed, ctx):
        dtype, shape = ctx
        return ops.adaq_decode_aggregate(tensor_compressed[0], 1, shape.numel(), self.compress_ratio,
                                         out_dtype=dtype).view(shape)

    def decode_aggregate_gathered(self, gathered, ctx, world_size):
        if not gathered[0].is_cuda:
            return None
        dtype, shape = ctx
        return ops.adaq_decode_aggregate(gathered[0], world_size, shape.numel(), self.compress_ratio,
                                         divisor=world_size if self.average else 1.0, out_dtype=dtype).view(shape)

    def fused_step(self, communicator, tensor, name):
        if not (communicator.__class__ is Allgather and communicator.memory.__class__ is NoneMemory
                and isinstance(tensor, torch.Tensor) and tensor.is_cuda and tensor.dtype in (ops.F32, ops.BF16)):
            return None
        world = int(communicator.world_size)
        if world == 1:
            return ops.adaq_step_w1(tensor, self.compress_ratio)
        g = ops.dev_grad(tensor)
        gathered = _gather_flat(ops.adaq_compress(g, self.compress_ratio), world)
        return self.decode_aggregate_gathered([gathered], (g.dtype, tensor.shape), world)


def grace_from_params(params):
    """grace_amd.inceptionn.grace_from_params, plus ``'compressor': 'adaq'`` with the optional key
    ``compress_ratio`` (0.01); memory and communicator as there."""
    from grace_amd.inceptionn import grace_from_params as base_from_params
    if params.get('compressor', 'none') != 'adaq':
        return base_from_params(params)
    compressor = AdaqCompressor(params.get('compress_ratio', 0.01))
    comm = base_from_params({**params, 'compressor': 'none'})   # the memory and the communicator
    comm.compressor = compressor
    return comm
