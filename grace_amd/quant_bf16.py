"""QSGD and TernGrad over Allgather on bfloat16 gradients.

``QSGDCompressor``, ``QSGDCompressor_CUDA`` and ``TernGradCompressor`` here are grace_amd.dist's
classes with the bfloat16 dispatch added: use them in their place, with the same constructor
arguments,

    from grace_amd.quant_bf16 import QSGDCompressor
    comm = Allgather(QSGDCompressor(127), NoneMemory(), world_size)

A float32 gradient takes the parent class's path unchanged.  ``Allgather(..., NoneMemory()).step``
on a CUDA bfloat16 tensor reads the gradient as it is, at every world size: the codes, bucket norms
and scalars on the wire are what the f32 class sends for ``g.float()`` under the same name and step
(the parent's ``_uniforms`` draws them, so ``rng="torch_cpu"`` works and f32 and bf16 ranks can
share a wire), and the result is a new bf16 tensor of the gradient's shape: the f32 result rounded
once to nearest even, at world > 1 after the rank-ordered sum and the division.

Only ``fused_step`` is overridden.  ``compress`` by hand on bf16 still raises TypeError, so AllToAll
and ResidualMemory keep refusing bf16; QSGD on bf16 needs ``bucket_size == 128``; float16 raises
TypeError.
"""
import torch

from grace_amd import ops
from grace_amd._bf16 import bf16_on_allgather
from grace_amd.dist.communicator.allgather import _gather_flat
from grace_amd.dist.compressor.qsgd import QSGDCompressor as _F32QSGDCompressor
from grace_amd.dist.compressor.qsgd import QSGDCompressor_CUDA as _F32QSGDCompressor_CUDA
from grace_amd.dist.compressor.terngrad import TernGradCompressor as _F32TernGradCompressor
from grace_amd.dist.memory.none import NoneMemory

BF16 = torch.bfloat16


def _flat_aligned(tensor):
    """The gradient flat, contiguous and 8-byte aligned (a view where it already is so)."""
    g = ops.dev_grad(tensor)
    return g.clone() if g.data_ptr() % 8 else g


class _QSGDBf16:
    """fused_step of both QSGD flavours (mixed in ahead of the f32 class)."""

    def fused_step(self, communicator, tensor, name):
        if not bf16_on_allgather(communicator, tensor, NoneMemory):
            return super().fused_step(communicator, tensor, name)
        if int(self.bucket_size) != 128:
            raise TypeError(f"grace_amd: QSGD on a bfloat16 gradient needs bucket_size 128, got {self.bucket_size} "
                            "(other bucket sizes are float32 only)")
        g = _flat_aligned(tensor)
        n, world = g.numel(), int(communicator.world_size)
        u, seed = self._uniforms(n, name, g.device)
        if world == 1:
            return ops.qsgd_step_w1(g, self.quantum_num, variant=self.variant, u=u, seed=seed).view(tensor.shape)
        codes, norms = ops.qsgd_compress(g, self.quantum_num, 128, variant=self.variant, u=u, seed=seed)
        codes, norms = _gather_flat(codes, world), _gather_flat(norms, world)
        return ops.qsgd_decompress(codes, norms, self.quantum_num, 128, n, variant=self.variant, world=world,
                                   aggregate=True, divisor=world if self.average else 1.0,
                                   out_dtype=BF16).view(tensor.shape)


class QSGDCompressor(_QSGDBf16, _F32QSGDCompressor):
    pass


class QSGDCompressor_CUDA(_QSGDBf16, _F32QSGDCompressor_CUDA):
    pass


class TernGradCompressor(_F32TernGradCompressor):

    def fused_step(self, communicator, tensor, name):
        if not bf16_on_allgather(communicator, tensor, NoneMemory):
            return super().fused_step(communicator, tensor, name)
        g = _flat_aligned(tensor)
        n, world = g.numel(), int(communicator.world_size)
        u, seed = self._uniforms(n, name, g.device)
        if world == 1:   # the wire format does not matter here
            return ops.terngrad_step_w1(g, u=u, seed=seed).view(tensor.shape)
        codes, scalar = ops.terngrad_compress(g, u=u, seed=seed)
        if self.wire == "2bit":
            packed = _gather_flat(ops.tern_pack(codes), world).view(world, -1)
            codes = torch.cat([ops.tern_unpack(packed[r], n) for r in range(world)])
        else:
            codes = _gather_flat(codes, world)
        scalars = _gather_flat(scalar, world)
        return ops.terngrad_decompress(codes, scalars, n, world=world, aggregate=True,
                                       divisor=world if self.average else 1.0, out_dtype=BF16).view(tensor.shape)
