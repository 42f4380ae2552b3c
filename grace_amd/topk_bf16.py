"""Top-k over Allgather on bfloat16 gradients.

``TopKCompressor`` here is grace_amd.dist's TopKCompressor with the bfloat16 dispatch added: use it in
its place, with the same Allgather communicator and ResidualMemory / NoneMemory,

    from grace_amd.topk_bf16 import TopKCompressor
    comm = Allgather(TopKCompressor(0.01), ResidualMemory(), world_size)

A float32 gradient takes the parent class's path unchanged (every f32 call goes to it as it is, so
f32 results, buffers and timings are the parent's).  A bfloat16 gradient is read as it is: the
payload, the residual, its spare buffer and the carry are f32, bit-identical to what the f32 path
gives for ``g.float()``; the dense result has the gradient's dtype and shape and is the f32 result
rounded once to nearest even -- at world > 1 after the rank-ordered sum and the division, in the
decode's epilogue (grace_sparse_aggregate_sorted_bf16).  float16 still raises TypeError.
"""
import torch

from grace_amd import ops
from grace_amd._bf16 import bf16_on_allgather, exchange_decode_sorted
from grace_amd.dist.compressor.topk import TopKCompressor as _F32TopKCompressor
from grace_amd.dist.memory.none import NoneMemory
from grace_amd.dist.memory.residual import ResidualMemory

BF16 = torch.bfloat16


class TopKCompressor(_F32TopKCompressor):

    def compress(self, tensor, name):
        """f32 or bf16 in; the payload is f32 values and int32 indices either way, so `decompress`
        is the parent's and decodes to f32."""
        flat = ops.dev_grad(tensor, "tensor")
        k = ops.ratio_k(flat.numel(), self.compress_ratio)
        _, vals, idx = ops.topk_compress(flat, k)
        if self.check_sync:
            ops.topk_check()
        return [vals, idx], tensor.size()

    def _fused_step(self, communicator, tensor, name):
        if not bf16_on_allgather(communicator, tensor, NoneMemory, ResidualMemory):
            return super()._fused_step(communicator, tensor, name)
        mem = communicator.memory
        g = ops.dev_grad(tensor)
        n = g.numel()
        k = ops.ratio_k(n, self.compress_ratio)
        world = int(communicator.world_size)
        divisor = world if self.average else 1
        if type(mem) is NoneMemory:
            if world == 1:   # payload and (0 + d) / 1 from one read of the tensor; never recycled
                return ops.topk_step_dense(g, k)[3].view(tensor.shape)
            # the unfused path cannot return bf16 (ctx = tensor.size() carries no dtype)
            buf, _, _ = ops.topk_compress(g, k)
            return exchange_decode_sorted(buf, k, n, world, divisor).view(tensor.shape)
        # the residual is f32 whatever the gradient's dtype; one of another dtype or size does not count
        # (no contiguity test, unlike ops._f32_residual: a strided f32 one counts here and is refused
        # with ValueError by the step below, where that rule would restart the name without a word)
        res = mem.residuals.get(name)
        has = res is not None and res.dtype == torch.float32 and res.numel() == n and res.device == g.device
        if not has:
            # the buffer this step writes the name's first residual into (no second one at world > 1)
            res = torch.empty(n, dtype=torch.float32, device=g.device)
        carry, carry_valid = mem.carry_for(name, res, has, k)
        if world == 1:
            # a new bf16 result every step: no recycling (recycle_output="always" included), no
            # placement probe (ops.pick_pair), no kept output buffer and no line map
            out = torch.empty_like(g)
            ops.topk_residual_step(g, res, has, mem.beta, mem.gamma, k, out=out, carry=carry,
                                   carry_valid=carry_valid)
            mem.residuals[name] = res
            mem.carry_written(name, res, carry)
            return out.view(tensor.shape)
        if getattr(mem, "keep_spare", True):
            # the spare is asked for with the f32 residual as its model (spare_for allocates like its
            # argument, and its reuse test does not look at the dtype), so it is f32 with n elements
            res_new = mem.spare_for(name, res) if has else res
            if res_new.dtype != torch.float32:
                res_new = torch.empty_like(res)
            buf, _, _ = ops.topk_residual_step_swap(g, res if has else None, has, mem.beta, mem.gamma, k, res_new,
                                                    carry=carry, carry_valid=carry_valid)
            mem.retire(name, res if has else None)
            mem.residuals[name] = res_new
            mem.carry_written(name, res_new, carry)
        else:
            buf, _, _ = ops.topk_residual_step(g, res, has, mem.beta, mem.gamma, k, out=None, carry=carry,
                                               carry_valid=carry_valid)
            mem.residuals[name] = res
            mem.carry_written(name, res, carry)
        return exchange_decode_sorted(buf, k, n, world, divisor).view(tensor.shape)
