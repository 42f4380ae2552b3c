"""Deep Gradient Compression over Allgather on bfloat16 gradients.

``DgcCompressor`` here is grace_amd.dist's class with the bfloat16 dispatch added: use it in its
place, with the same constructor arguments, the same Allgather and the same DgcMemory,

    from grace_amd.dgc_bf16 import DgcCompressor
    comm = Allgather(DgcCompressor(0.01), DgcMemory(0.9, False, world_size), world_size)

A float32 gradient takes the parent class's path unchanged.  ``Allgather(..., DgcMemory).step`` on a
CUDA bfloat16 tensor reads the gradient as it is, at every world size.  The momentum state
(``mem.residuals[name]``, ``mem.gradients[name]``) stays f32 and is bit for bit what the f32 class
leaves for ``g.float()``, so bf16 and f32 steps of one name share it; the sample, the thresholds,
the counts and the records on the wire are the f32 class's too (f32 and bf16 ranks can share a
wire).  The result is a new bf16 tensor of the gradient's shape: the f32 result rounded once to
nearest even, at world > 1 after the rank-ordered sum and the division.

  * world 1, no clipping: one fused pass (grace_dgc_step_w1_fused_bf16), 20 B per element;
  * world 1 with ``gradient_clipping``: bf16 sum of squares, clip to f32, then the f32 compensate,
    select and a mask pass that writes bf16;
  * world > 1: the bf16 compensate (or, with clipping, the clip to f32 and the f32 compensate) into
    the memory's own f32 buffers, then the parent's exchange with the decode that writes bf16
    (grace_sparse_aggregate_records_bf16): counts, capacity, retry and defer modes, ``host_reads``,
    ``overflows`` and the capacity growth are the parent's, step for step.  A tensor of 2^31
    elements or more raises ValueError (the parent hands those to its generic path, which takes no
    bf16).

Only ``fused_step`` and ``_exchange_step`` are overridden; the compensate and the clipping of a bf16
step live here because grace_amd/dist/ is as it was.  ``compress`` / ``decompress`` and
``DgcMemory.compensate`` / ``update`` by hand on bf16 still raise TypeError, and so does float16.
"""
import torch
import torch.distributed as dist

from grace_amd import ops
from grace_amd._bf16 import bf16_on_allgather
from grace_amd.dist.compressor.dgc import DgcCompressor as _F32DgcCompressor
from grace_amd.dist.memory.dgc import DgcMemory

BF16 = torch.bfloat16
MAX_EXCHANGE_N = 2 ** 31   # grace_dgc_write_capped and the records decode index with int32


class DgcCompressor(_F32DgcCompressor):
    def fused_step(self, communicator, tensor, name):
        if not bf16_on_allgather(communicator, tensor, DgcMemory):
            return super().fused_step(communicator, tensor, name)
        mem = communicator.memory
        W = int(communicator.world_size)
        g = ops.dev_grad(tensor)
        n = g.numel()
        if W > 1 and n >= MAX_EXCHANGE_N:
            raise ValueError(f"grace_amd: DGC on a bfloat16 gradient at world size > 1 takes fewer than 2^31 elements, "
                             f"got {n}")
        res, acc = mem.residuals.get(name), mem.gradients.get(name)
        has = ops._f32_residual(res, n, g.device) and ops._f32_residual(acc, n, g.device)
        if W == 1 and not mem.gradient_clipping:
            sidx, seed = self._sampling(g, name)
            out, r_new, a_new = ops.dgc_step_w1_fused(g, res if has else None, acc if has else None, has,
                                                      mem.momentum, self.compress_ratio, sample_idx=sidx, seed=seed)
            mem.residuals[name], mem.gradients[name] = r_new, a_new
            return out.view(tensor.shape)
        if mem.gradient_clipping:
            # DgcMemory.compensate's clipping; the clipped gradient is f32 (its bound is no bf16 number)
            s = ops.sumsq(g)
            if dist.is_available() and dist.is_initialized():
                dist.all_reduce(s)
            g = ops.clip_by_sumsq(g, s, mem.world_size)
        if not has:
            res = mem.residuals[name] = torch.empty(n, dtype=torch.float32, device=g.device)
            acc = mem.gradients[name] = torch.empty(n, dtype=torch.float32, device=g.device)
        ops.dgc_compensate(g, res, acc, has, mem.momentum)   # the bf16 form unless clipped
        sidx, seed = self._sampling(acc, name)
        if W == 1:
            ws = ops.dgc_select(acc, self.compress_ratio, sample_idx=sidx, seed=seed)
            return ops.dgc_step_w1(acc, res, acc, ws, out_dtype=BF16).view(tensor.shape)
        return self._exchange_step(acc, name, mem, W, sidx, seed, out_dtype=BF16).view(tensor.shape)

    def _exchange_step(self, t, name, mem, W, sidx, seed, out_dtype=torch.float32):
        """The parent's _exchange_step, line for line, with `out_dtype` handed to its two decodes (the
        parent has no hook there; tests/test_abi_dgc_bf16.py holds the two bodies together)."""
        n = t.numel()
        dev = t.device
        divisor = W if self.average else 1
        ws = ops.dgc_threshold_dev(t, self.compress_ratio, sample_idx=sidx, seed=seed)
        res, acc = mem.residuals[name], mem.gradients[name]
        defer = self.exchange == "capacity" and self.overflow == "defer"
        if defer:
            self._settle(name, n)
        cap = self.capacity.get(name) if self.exchange == "capacity" else None
        stat = torch.empty(2, dtype=torch.int32, device=dev)
        if cap is not None and cap <= n:
            rec, recs = self._records(t, ws, cap, W)
            out = ops.sparse_aggregate_capped(recs, cap, W, n, divisor, stat, out_dtype=out_dtype)
            if defer:
                ops.dgc_mask_update_capped(rec, cap, res, acc)
                pinned = torch.empty(2, dtype=torch.int32, pin_memory=True)
                pinned.copy_(stat, non_blocking=True)
                ev = torch.cuda.Event()
                ev.record()
                self._pending[name] = (pinned, ev)
                return out
            self.host_reads += 1
            mx, over = (int(v) for v in stat.cpu().tolist())        # one read, after the exchange
            if not over:
                ops.dgc_mask_update_capped(rec, cap, res, acc)
                if self._grow(mx, n) * 4 < cap:
                    self.capacity[name] = self._grow(mx, n)
                return out
            self.overflows += 1                                      # retry: memory still untouched
        # counts exchange: the W device counts, ONE host read, then records sized to the largest
        cnt = ws[8:12].view(torch.int32)
        counts_dev = torch.empty(W, dtype=torch.int32, device=dev)
        dist.all_gather_into_tensor(counts_dev, cnt)
        self.host_reads += 1
        mx = max(int(c) for c in counts_dev.cpu().tolist())
        cap_exact = max(mx, 1)
        rec, recs = self._records(t, ws, cap_exact, W)
        out = ops.sparse_aggregate_capped(recs, cap_exact, W, n, divisor, stat, out_dtype=out_dtype)
        ops.dgc_mask_update_capped(rec, cap_exact, res, acc)
        if self.exchange == "capacity":
            self.capacity[name] = self._grow(mx, n)
        return out
