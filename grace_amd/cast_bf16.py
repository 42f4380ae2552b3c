"""Natural compression, fp16 and one-bit over Allgather on bfloat16 gradients.

``NaturalCompressor``, ``NaturalCompressor_CUDA``, ``FP16Compressor`` and ``OneBitCompressor`` here
are grace_amd.dist's classes with the bfloat16 dispatch added: use them in their place, with the same
constructor arguments,

    from grace_amd.cast_bf16 import FP16Compressor
    comm = Allgather(FP16Compressor(), NoneMemory(), world_size)

A float32 gradient takes the parent class's path unchanged.  ``Allgather(..., NoneMemory()).step``
on a CUDA bfloat16 tensor reads the gradient as it is, at every world size: the u8 codes, the f16
payload and one-bit's mask0 on the wire are bit for bit what the f32 class sends for ``g.float()``
under the same name and step (the parent's generators and step counter are used, so
``rng="torch_cpu"`` and ``"deterministic"`` work and f32 and bf16 ranks can share a wire), gathered
by the parent's collectives in the parent's order.  One-bit's two means are the same formula on f64
sums taken over another partition than the f32 class's encode, so they can differ from that class's
in the last ulp (both are within 2 ulp of the formula on the exact sums); the result is exact given
the means sent.  The result is a new bf16 tensor of the gradient's shape: the f32 result ((0 + d_0) + d_1 + ...) / divisor rounded once to nearest even.  (The reference would sum
bf16 tensors in bf16; this sums in f32 and rounds once.)

Only ``fused_step`` is overridden.  ``compress`` and ``decompress`` by hand on bf16 still raise
TypeError, so AllToAll, ResidualMemory, the Horovod flavour and ``grace_from_params`` keep refusing
bf16; float16 raises TypeError.
"""
import torch

from grace_amd import ops
from grace_amd._bf16 import bf16_on_allgather
from grace_amd.dist.communicator.allgather import _gather_flat
from grace_amd.dist.compressor.fp16 import FP16Compressor as _F32FP16Compressor
from grace_amd.dist.compressor.natural import NaturalCompressor as _F32NaturalCompressor
from grace_amd.dist.compressor.natural import NaturalCompressor_CUDA as _F32NaturalCompressor_CUDA
from grace_amd.dist.compressor.onebit import OneBitCompressor as _F32OneBitCompressor
from grace_amd.dist.memory.none import NoneMemory

BF16 = torch.bfloat16


def _flat_aligned(tensor):
    """The gradient flat, contiguous and 16-byte aligned (a view where it already is so)."""
    g = ops.dev_grad(tensor)
    return g.clone() if g.data_ptr() % 16 else g


class _NaturalBf16:
    """fused_step of both natural flavours (mixed in ahead of the f32 class)."""

    def fused_step(self, communicator, tensor, name):
        if not bf16_on_allgather(communicator, tensor, NoneMemory):
            return super().fused_step(communicator, tensor, name)
        g = _flat_aligned(tensor)
        n, world = g.numel(), int(communicator.world_size)
        mode = self._w1_mode()
        if world == 1 and mode is not None:   # the parent's fused step: its counter, its seed
            self._step += 1
            return ops.cast_step_w1(g, mode, self._w1_seed(name)).view(tensor.shape)
        codes = _gather_flat(self._encode(g, name), world)   # the parent's draw, counter and seed
        return ops.natural_decompress(codes, n, self.flavour, world=world, aggregate=True,
                                      divisor=world if self.average else 1.0, out_dtype=BF16).view(tensor.shape)


class NaturalCompressor(_NaturalBf16, _F32NaturalCompressor):
    pass


class NaturalCompressor_CUDA(_NaturalBf16, _F32NaturalCompressor_CUDA):
    pass


class FP16Compressor(_F32FP16Compressor):

    def fused_step(self, communicator, tensor, name):
        if not bf16_on_allgather(communicator, tensor, NoneMemory):
            return super().fused_step(communicator, tensor, name)
        g = _flat_aligned(tensor)
        n, world = g.numel(), int(communicator.world_size)
        if world == 1:
            return ops.cast_step_w1(g, 3, 0).view(tensor.shape)
        h = _gather_flat(ops.fp16_compress(g), world)
        return ops.fp16_decompress_aggregate(h, n, world, divisor=world if self.average else 1.0,
                                             out_dtype=BF16).view(tensor.shape)


class OneBitCompressor(_F32OneBitCompressor):

    def fused_step(self, communicator, tensor, name):
        if not bf16_on_allgather(communicator, tensor, NoneMemory):
            return super().fused_step(communicator, tensor, name)
        g = _flat_aligned(tensor)
        n, world = g.numel(), int(communicator.world_size)
        if world == 1:
            return ops.onebit_step_w1(g, quirk=self.compat_uint8_not)[1].view(tensor.shape)
        mask0, means = ops.onebit_encode_grad(g)
        # the parent's three gathers, in its payload's order: mask0, mean0, mean1
        mask0, mean0, mean1 = (_gather_flat(t, world) for t in (mask0, means[0:1], means[1:2]))
        return ops.onebit_decode_aggregate(mask0, mean0, mean1, world, n, quirk=self.compat_uint8_not,
                                           divisor=world if self.average else 1.0,
                                           out_dtype=BF16).view(tensor.shape)
