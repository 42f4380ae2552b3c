"""Shared by the bfloat16 stand-in modules: the test for a step they take, and the top-k decode tail."""
import torch
import torch.distributed as dist

from grace_amd import ops
from grace_amd.dist.communicator.allgather import Allgather


def bf16_on_allgather(communicator, tensor, *memory_types):
    """Whether this is a step of a CUDA bfloat16 tensor on an Allgather whose memory is exactly one
    of `memory_types` (a subclass of one does not count)."""
    return (isinstance(communicator, Allgather) and type(communicator.memory) in memory_types
            and isinstance(tensor, torch.Tensor) and tensor.is_cuda and tensor.dtype == ops.BF16)


def exchange_decode_sorted(buf, k, n, world, divisor, out=None):
    """The world > 1 tail of a bf16 top-k step: this rank's packed f32 payload `buf` ([vals f32[k] |
    idx i32[k]], indices into n elements) -> the flat rank-ordered aggregate
    ((0 + d_0) + d_1 + ...) / divisor, rounded once to bfloat16 after the sum and the division, in
    `out` when given.  (The f32 tail of dist/compressor/topk.py is these steps with an f32 result.)"""
    if n > ops.SORT_PAYLOAD_MAX_N:
        # beyond the grouping's range: the scatter accumulates in f32, so a second pass narrows it
        gathered = torch.empty(world * 2 * k, dtype=torch.float32, device=buf.device)
        dist.all_gather_into_tensor(gathered, buf)
        dense = ops.sparse_aggregate(gathered, gathered[k:].view(torch.int32), 2 * k, [k] * world, world, n, divisor)
        return ops.f32_to_bf16(dense, out=out)
    # grouped by output chunk, one all-gather, one decode that writes every element (payload.hip)
    sbuf = ops.sort_payload(buf, k, n)
    gathered = torch.empty(world * sbuf.numel(), dtype=torch.float32, device=buf.device)
    dist.all_gather_into_tensor(gathered, sbuf)
    return ops.sparse_aggregate_sorted(gathered, k, world, n, divisor, out_dtype=ops.BF16, out=out)
