"""The sign family over Allgather on bfloat16 gradients.

``SignSGDCompressor``, ``SignumCompressor`` and ``EFSignSGDCompressor`` here are grace_amd.dist's
classes with the bfloat16 dispatch added: use them in their place, with the same constructor
arguments, communicator and memory,

    from grace_amd.sign_bf16 import EFSignSGDCompressor
    comm = Allgather(EFSignSGDCompressor(lr), EFSignSGDMemory(lr), world_size)

A float32 gradient takes the parent class's path unchanged.  A bfloat16 gradient is read as it is:
codes, words, the Signum momentum and the EF-signSGD residual and mean are what the f32 path gives
for ``g.float()`` (the state stays f32, so f32 and bf16 steps of one name share it); the dense
result has the gradient's dtype and shape -- +-1 for signSGD and Signum, and for EF-signSGD the f32
result rounded once to nearest even, at world > 1 after the rank-ordered sum and the division.
float16 still raises TypeError.

The EF-signSGD step on bf16 is fused (grace_efsign_step_bf16: two launches at world 1, against the
eight of the f32 class's compensate / compress / update / send_receive); the f32 class keeps its
unfused path.
"""
import torch

from grace_amd import ops
from grace_amd._bf16 import bf16_on_allgather
from grace_amd.dist.communicator.allgather import _gather_flat
from grace_amd.dist.compressor.efsignsgd import EFSignSGDCompressor as _F32EFSignSGDCompressor
from grace_amd.dist.compressor.signsgd import SignSGDCompressor as _F32SignSGDCompressor
from grace_amd.dist.compressor.signum import SignumCompressor as _F32SignumCompressor
from grace_amd.dist.memory.efsignsgd import EFSignSGDMemory
from grace_amd.dist.memory.none import NoneMemory

BF16 = torch.bfloat16
F32 = torch.float32


class SignSGDCompressor(_F32SignSGDCompressor):
    """`compress` is the parent's (ops.sign_encode / sign_encode_bits take bf16; `decompress` decodes
    to f32); the step on a bf16 tensor returns bf16 at every world size, with both wires."""

    def fused_step(self, communicator, tensor, name):
        if not bf16_on_allgather(communicator, tensor, NoneMemory):
            return super().fused_step(communicator, tensor, name)
        world = int(communicator.world_size)
        if world == 1:
            # as the f32 step: one launch into a buffer reused only when the caller dropped the last one
            if not tensor.is_contiguous():
                return ops.sign_step_w1(tensor, want_codes=False, reuse_out=True)[1].view(tensor.shape)
            out = ops.reusable_output("sign_w1", tensor.shape, BF16, tensor.device)
            ops.launch_sign_step_w1(tensor, out)
            return out
        n = tensor.numel()
        if self.wire == "bits":
            words = _gather_flat(ops.sign_encode_bits(tensor), world)
            return ops.sign_majority_bits(words, world, n, out_dtype=BF16).view(tensor.shape)
        codes = _gather_flat(ops.sign_encode(tensor), world)
        return ops.sign_majority(codes, world, n, out_dtype=BF16).view(tensor.shape)


class SignumCompressor(_F32SignumCompressor):

    def compress(self, tensor, name):
        """f32 goes to the parent; bf16 updates the same f32 momentum buffer (a stored buffer of
        another dtype, size or device does not count: the step is then a first step)."""
        if not (isinstance(tensor, torch.Tensor) and tensor.dtype == BF16):
            return super().compress(tensor, name)
        g = ops.dev_grad(tensor)
        buf = self.momentums.get(name)
        has_prev = buf is not None and ops._f32_residual(buf, g.numel(), g.device)
        if not has_prev:
            buf = torch.empty(g.numel(), dtype=F32, device=g.device)
        codes = ops.signum_encode(g, buf, has_prev, self.momentum)
        self.momentums[name] = buf
        return [codes], tensor.size()

    def fused_step(self, communicator, tensor, name):
        if not bf16_on_allgather(communicator, tensor, NoneMemory):
            return super().fused_step(communicator, tensor, name)
        world = int(communicator.world_size)
        (codes,), _ = self.compress(tensor, name)
        return ops.sign_majority(_gather_flat(codes, world), world, tensor.numel(), out_dtype=BF16).view(tensor.shape)


class EFSignSGDCompressor(_F32EFSignSGDCompressor):

    def fused_step(self, communicator, tensor, name):
        """Allgather(EFSignSGDCompressor, EFSignSGDMemory).step on a bf16 tensor: the residual lives in
        memory.residuals[name] as f32 and is updated in place; any other triple or tensor is the
        parent's (an f32 gradient takes its unfused path, on the same residual)."""
        if not bf16_on_allgather(communicator, tensor, EFSignSGDMemory):
            return super().fused_step(communicator, tensor, name)
        mem = communicator.memory
        g = ops.dev_grad(tensor)
        n = g.numel()
        world = int(communicator.world_size)
        res = mem.residuals.get(name)
        has = res is not None and ops._f32_residual(res, n, g.device)
        if not has:
            res = torch.empty(n, dtype=F32, device=g.device)   # the name's first residual is written here
        if world == 1:
            out = torch.empty_like(g)
            ops.efsign_step(g, res, has, mem.learning_rate, self.learning_rate, want_codes=False, out=out)
            mem.residuals[name] = res
            return out.view(tensor.shape)
        mean, codes, _ = ops.efsign_step(g, res, has, mem.learning_rate, self.learning_rate, want_codes=True)
        mem.residuals[name] = res
        # the parent's payload: mean f32[1] and the u8 codes, one all-gather each
        means, codes = _gather_flat(mean, world), _gather_flat(codes, world)
        out = ops.efsign_decode_aggregate(means, codes, world, n, self.learning_rate, out_dtype=BF16)
        return out.view(tensor.shape)
