"""Quantile-bucket quantisation (SketchML: Jiang, Fu, Yang and Cui, SIGMOD 2018;
grace_dl/tensorflow/compressor/sketch.py): the tensor is cut into ``quantiles`` equal-mass buckets at
its own quantiles, every element sends its bucket number and decodes to the bucket's mean.
Data-adaptive, stateless and fixed rate: n bytes of codes, or n / 2 at 16 buckets and fewer, plus 4
bytes a bucket of means, the same for a float32 and a bfloat16 gradient.  The arithmetic is stated in
include/grace_hip_sketch.h.

Two deliberate departures from the reference file.  It interpolates each edge linearly between the two
neighbouring order statistics; here an edge is the lower of the two, ``sorted(x)[j * (n - 1) // Q]``,
so every edge is an element of the tensor, found exactly by a radix multi-select, and the edges and the
codes are reproducible bit for bit.  It sends 16-bit codes from 256 buckets on; here 2 to 256 buckets
are served, a code is one byte, and two codes share a byte at 16 buckets and fewer.

``Allgather(SketchCompressor(Q), NoneMemory(), W).step`` on a CUDA float32 or bfloat16 tensor is
fused at every world size and returns the gradient's dtype.  ``compress`` / ``decompress`` by hand, and
so ResidualMemory, take float32; bfloat16 there and float16 anywhere raise TypeError.  AllToAll is
not served.

``grace_from_params`` below is grace_amd.u8bit's (and so grace_amd.dist's) with the key ``'sketch'``
and its ``quantiles`` (16) added; every other params dict is handed on unchanged.
"""
import torch

from grace_amd import ops
from grace_amd.dist import Compressor
from grace_amd.dist.communicator.allgather import Allgather, _gather_flat
from grace_amd.dist.memory.none import NoneMemory


class SketchCompressor(Compressor):

    def __init__(self, quantiles=16):
        super().__init__(tensors_size_are_same=True)
        self.quantiles = ops._sketch_q(quantiles, "SketchCompressor")

    def compress(self, tensor, name):
        flat = ops.dev_f32(tensor)
        codes, means = ops.sketch_compress(flat, self.quantiles)
        return [codes, means], (tensor.dtype, tensor.size())

    def decompress(self, tensor_compressed, ctx):
        codes, means = tensor_compressed
        dtype, shape = ctx
        return ops.sketch_decode_aggregate(codes, means, 1, shape.numel(), self.quantiles,
                                           out_dtype=dtype).view(shape)

    def decode_aggregate_gathered(self, gathered, ctx, world_size):
        codes, means = gathered
        if not codes.is_cuda:
            return None
        dtype, shape = ctx
        return ops.sketch_decode_aggregate(codes, means, world_size, shape.numel(), self.quantiles,
                                           divisor=world_size if self.average else 1.0,
                                           out_dtype=dtype).view(shape)

    def fused_step(self, communicator, tensor, name):
        if not (communicator.__class__ is Allgather and communicator.memory.__class__ is NoneMemory
                and isinstance(tensor, torch.Tensor) and tensor.is_cuda and tensor.dtype in (ops.F32, ops.BF16)):
            return None
        world = int(communicator.world_size)
        if world == 1:
            return ops.sketch_step_w1(tensor, self.quantiles)[1]
        g = ops.dev_grad(tensor)
        codes, means = ops.sketch_compress(g, self.quantiles)
        codes, means = _gather_flat(codes, world), _gather_flat(means, world)
        return ops.sketch_decode_aggregate(codes, means, world, g.numel(), self.quantiles,
                                           divisor=world if self.average else 1.0,
                                           out_dtype=g.dtype).view(tensor.shape)


def grace_from_params(params):
    """grace_amd.u8bit.grace_from_params, plus ``'compressor': 'sketch'`` with the optional key
    ``quantiles`` (16); memory and communicator as there."""
    from grace_amd.u8bit import grace_from_params as base_from_params
    if params.get('compressor', 'none') != 'sketch':
        return base_from_params(params)
    compressor = SketchCompressor(params.get('quantiles', 16))
    comm = base_from_params({**params, 'compressor': 'none'})   # the memory and the communicator
    comm.compressor = compressor
    return comm
