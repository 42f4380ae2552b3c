"""Error-bounded variable-width compression (INCEPTIONN: Li, Park, Alian, Yuan, Qu, Pan, Wang,
Schwing, Esmaeilzadeh and Kim, MICRO 2018; grace_dl/tensorflow/compressor/inceptionn.py): an element
travels in 0, 8, 16 or 32 bits, chosen by its exponent, behind a 2-bit tag.  With ``bound_bits`` = b no
element below 1 in magnitude moves by 2^-b or more, and every other element arrives bit for bit: a
per-element guarantee, at a rate the data decides (a normal gradient of scale 1e-3 at b = 10 sends 14 %
of its float32 bytes).  Stateless; the wire is the same for a float32 and a bfloat16 gradient.  The
arithmetic and the wire are stated in include/grace_hip_inceptionn.h.

Deliberate departures from the reference file.  It derives its exponent threshold from ``log10`` of a
decimal bound; here the argument is the exponent itself, the bound 2^-b.  Its 16-bit and 8-bit codes
leave their top magnitude bit always zero (at its default bound the 8-bit code is 0 or 1); here the
codes are scaled to use their bits.  Its tags are interleaved in four quarters of the tensor; here they
are in element order.  It sends four tensors; here the payload is one byte stream in tiles of 4096
elements behind a tile directory, so the decoder is parallel.

The payload's length depends on the data, so ``compress`` reads one word back from the device, and the
exchange is Allgather's size exchange followed by a padded all-gather.
``Allgather(InceptionnCompressor(b), NoneMemory(), W).step`` on a CUDA float32 or bfloat16 tensor is
fused at every world size and returns the gradient's dtype.  ``compress`` / ``decompress`` by hand, and
so ResidualMemory, take float32; bfloat16 there and float16 anywhere raise TypeError.  AllToAll, the
sharded engines and the Horovod optimizer path are not served, and there is no capacity-sized exchange
that would avoid the host read.

``grace_from_params`` below is grace_amd.sketch's (and so grace_amd.dist's) with the key
``'inceptionn'`` and its ``bound_bits`` (10) added; every other params dict is handed on unchanged.
"""
import torch

from grace_amd import ops
from grace_amd.dist import Compressor
from grace_amd.dist.communicator.allgather import Allgather
from grace_amd.dist.memory.none import NoneMemory


class InceptionnCompressor(Compressor):

    def __init__(self, bound_bits=10):
        super().__init__(tensors_size_are_same=False)
        self.bound_bits = ops._inceptionn_b(bound_bits, "InceptionnCompressor")

    def compress(self, tensor, name):
        payload = ops.inceptionn_compress(ops.dev_f32(tensor), self.bound_bits)
        return [payload[:ops.inceptionn_payload_bytes(payload)]], (tensor.dtype, tensor.size())

    def decompress(self, tensor_compressed, ctx):
        dtype, shape = ctx
        return ops.inceptionn_decode_aggregate(tensor_compressed[0], 1, shape.numel(), self.bound_bits,
                                               out_dtype=dtype).view(shape)

    def decode_aggregate_variable(self, gathered, sizes, ctx, world_size):
        """every rank's payload sits at a multiple of the longest one's length, itself a multiple of 16"""
        if not gathered[0].is_cuda:
            return None
        dtype, shape = ctx
        return ops.inceptionn_decode_aggregate(gathered[0], world_size, shape.numel(), self.bound_bits,
                                               divisor=world_size if self.average else 1.0,
                                               out_dtype=dtype).view(shape)

    def fused_step(self, communicator, tensor, name):
        if not (communicator.__class__ is Allgather and communicator.memory.__class__ is NoneMemory
                and isinstance(tensor, torch.Tensor) and tensor.is_cuda and tensor.dtype in (ops.F32, ops.BF16)):
            return None
        world = int(communicator.world_size)
        if world == 1:
            return ops.inceptionn_step_w1(tensor, self.bound_bits)
        g = ops.dev_grad(tensor)
        payload = ops.inceptionn_compress(g, self.bound_bits)
        gathered, sizes = communicator._gather_variable([payload[:ops.inceptionn_payload_bytes(payload)]], world)
        return self.decode_aggregate_variable(gathered, sizes, (g.dtype, tensor.shape), world)


def grace_from_params(params):
    """grace_amd.sketch.grace_from_params, plus ``'compressor': 'inceptionn'`` with the optional key
    ``bound_bits`` (10); memory and communicator as there."""
    from grace_amd.sketch import grace_from_params as base_from_params
    if params.get('compressor', 'none') != 'inceptionn':
        return base_from_params(params)
    compressor = InceptionnCompressor(params.get('bound_bits', 10))
    comm = base_from_params({**params, 'compressor': 'none'})   # the memory and the communicator
    comm.compressor = compressor
    return comm
