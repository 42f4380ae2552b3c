"""Sharded top-k on bfloat16 shards with a bfloat16 dense result (DESIGN.md §9 "Sharded step").

``ShardedTopK`` here is grace_amd.dist.sharded.ShardedTopK with the bfloat16 path added: use it in
its place, with the same constructor arguments,

    from grace_amd.sharded_bf16 import ShardedTopK
    eng = ShardedTopK(0.001, group=group)
    dense = eng.step(shard, "bucket")

the way grace_amd.topk_bf16.TopKCompressor and grace_amd.segmented_bf16.SegmentedTopK stand in for
theirs: every file under grace_amd/dist/ is as it was.  A shard that is not bfloat16 is handed to the
parent class, so the f32 step is the parent's code (float16 and every dtype other than float32 and
bfloat16 raise TypeError).  A bfloat16 shard is read as it is by the local step
(grace_topk_residual_step_swap_bf16: 10 B per element instead of 12); the record, the exchange, the
residual, its spare buffer and the payload are f32 / int32, bit-identical to what the f32 step gives
for ``shard.float()``; the dense result is bfloat16 -- the f32 step's result rounded once to nearest
even, position by position (grace_shard_select_bf16; a NaN becomes 0x7FC0) -- zero-filled by
grace_fill_bf16 on the side stream, or, when the caller dropped the previous one, taken back and
cleared through its selection list (grace_shard_clear_bf16): 2 n bytes per rank instead of 4 n.

The plans, the residuals and their spares, the status words and their two-step parity, ``check()``,
``check_sizes``, ``last_payload``, ``host_reads`` and ``resizes`` are the parent's, shared by both
dtypes: a name whose shard changes dtype between steps keeps its residual and its plan.  Recycled
bf16 outputs and their selection lists are kept apart from the parent's f32 ones
(ops.OutputRecycler's key holds no dtype), so such a name is never handed a buffer of the other
dtype and never clears through the other dtype's list.

The parent class itself, given a bfloat16 shard, still runs the bf16 local step and returns an f32
dense result: bf16 users import this class.
"""
import torch
import torch.distributed as dist

from grace_amd import ops
from grace_amd.dist.sharded import NativeShardKernels as _NativeShardKernels
from grace_amd.dist.sharded import ShardedTopK as _ShardedTopK

F32 = torch.float32
BF16 = torch.bfloat16


class NativeShardKernels(_NativeShardKernels):
    """The parent's kernel set; the zero-fill takes a bfloat16 output as well (the select and the
    clear dispatch on the output's dtype in ops)."""

    def fill_zero(self, x):
        return ops.fill_bf16(x, 0) if x.dtype == BF16 else ops.fill(x, 0.0)


class ShardedTopK(_ShardedTopK):

    def __init__(self, compress_ratio, group=None, dense="replicated", kernels=None, check_sizes=False,
                 recycle_output=True):
        super().__init__(compress_ratio, group=group, dense=dense, kernels=kernels or NativeShardKernels(),
                         check_sizes=check_sizes, recycle_output=recycle_output)
        self._recycler_bf16 = ops.OutputRecycler()   # dropped bf16 results (the parent's holds the f32 ones)
        self._sel_bf16 = {}                          # name -> (its plan, two alternating sel_gi lists)

    def _plan(self, name, m, device, world, rank):
        before = self._plans.get(name)
        plan = super()._plan(name, m, device, world, rank)
        if plan is not before:
            # a new partition: the recycled bf16 output's selection was taken under the old one
            self._recycler_bf16.drop(name)
            self._sel_bf16.pop(name, None)
        return plan

    def _sel_buffer_bf16(self, name, plan, prev, device):
        """The sel_gi list this bf16 step's select writes: the plan's own pair belongs to the f32
        outputs, so the bf16 outputs of a name have a pair of their own; never the one `prev` (the
        recycled bf16 output's list, read by this step's clear) points at."""
        hit = self._sel_bf16.get(name)
        if hit is None or hit[0] is not plan:
            hit = self._sel_bf16[name] = (plan, [torch.empty(plan.world * plan.cap, dtype=torch.int32, device=device)
                                                 for _ in range(2)])
        pair = hit[1]
        return pair[1] if prev is pair[0] else pair[0]

    def _zero_out_bf16(self, out_len, device):
        """The parent's _zero_out for a bfloat16 output (grace_fill_bf16 on the side stream)."""
        K = self.k_ops
        if device.type != "cuda":
            return K.fill_zero(torch.empty(out_len, dtype=BF16, device=device)), None
        cur, side = self._side_stream(device)
        with torch.cuda.stream(side):
            out = torch.empty(out_len, dtype=BF16, device=device)
            K.fill_zero(out)
        out.record_stream(cur)
        return out, side

    def step(self, shard, name):
        if isinstance(shard, torch.Tensor) and shard.dtype not in (F32, BF16):
            raise TypeError(f"grace_amd: a shard must be float32 or bfloat16, got {shard.dtype}")
        if not isinstance(shard, torch.Tensor) or shard.dtype != BF16:
            return super().step(shard, name)
        # the parent's step with a bf16 output: the same order of calls on the same streams
        K = self.k_ops
        world, rank = self._world()
        g = shard.reshape(-1)
        dev = g.device
        m = g.numel()
        status, slot = self._check_status(dev)
        plan = self._plan(name, m, dev, world, rank)
        res = self.residuals.get(name)
        has_res = res is not None and res.numel() == m
        res_new = self._spare_residual(name, m, dev)    # f32, whatever the shard's dtype
        if not has_res:
            res = None
        out_len = m if self.dense == "shard" else plan.n
        out_base = plan.base if self.dense == "shard" else 0
        recycle = self.recycle_output and dev.type == "cuda"
        out = prev_sel = None
        if recycle:
            out, prev_sel = self._recycler_bf16.take(name, (out_len, dev), alloc=False)
        if out is not None and out.dtype == BF16 and prev_sel is not None \
                and prev_sel.numel() == plan.world * plan.cap:
            out, side = self._clear_out(out, out_base, prev_sel, dev)
        else:
            prev_sel = None
            out, side = self._zero_out_bf16(out_len, dev)
        sel = self._sel_buffer_bf16(name, plan, prev_sel, dev) if recycle else None
        rec = plan.record(m, dev, K.HDR)
        cap = plan.cap
        vals = rec[K.HDR:K.HDR + cap].view(F32)
        idx = rec[K.HDR + cap:K.HDR + 2 * cap]
        K.local_step(g, res, has_res, min(cap, m), vals, idx, res_new)
        if res is not None:
            st = res.untyped_storage()
            self._spare[name] = (res, st._cdata, st)
        self.residuals[name] = res_new
        res = res_new
        if world > 1:
            dist.all_gather_into_tensor(plan.recs, rec, group=self.group)
            recs = plan.recs
        else:
            recs = rec
        if side is not None:
            torch.cuda.current_stream(dev).wait_stream(side)
        if sel is None:
            K.select(recs, world, rank, cap, plan.tab, plan.k, res, out, out_base, plan.pay_idx, status)
        else:
            K.select(recs, world, rank, cap, plan.tab, plan.k, res, out, out_base, plan.pay_idx, status, sel)
            self._recycler_bf16.keep(name, out, sel)
        if dev.type == "cuda":
            ev = torch.cuda.Event()
            ev.record()
            self._slots(dev)[1][slot] = ev
        self._nstep += 1
        self.last_payload = (vals, plan.pay_idx)
        return out
