"""SegmentedTopK for bfloat16 (and float32) flat gradients (DESIGN.md §9 "Segmented step").

A subclass of grace_amd.dist.segmented.SegmentedTopK, used in its place -- with harness.GradBucket
and harness.step_segmented as before -- the way grace_amd.topk_bf16.TopKCompressor stands in for
grace_amd.dist's TopKCompressor: every file under grace_amd/dist/ is as it was, and a float32
gradient is handed to the parent class, so the f32 step is the parent's code.  For a bf16 flat
gradient every result is what the f32 segmented step produces for ``flat.float()``: the residual
(one f32 buffer), the payload (vals f32, idx int32, global indices) and the carry are bit-identical,
and the dense result is bf16, the f32 result rounded once to nearest even -- at world > 1 after the
rank-ordered sum and the division, in the decode's epilogue.  A name whose gradient changes dtype
between steps keeps its residual and its carry (the carry layout does not depend on the dtype).
"""
import torch

from grace_amd import _lib, ops
from grace_amd._bf16 import exchange_decode_sorted
from grace_amd.dist.segmented import SegmentedTopK as _SegmentedTopK

BF16 = torch.bfloat16


class SegmentedTopK(_SegmentedTopK):

    def tables_bf16(self, sizes, device, has_res, dense_out):
        """The parent's cached tables of this segment list with the main pass's chunk map
        (chk_off, chunk_li, nchunks) rebuilt for the bf16 kernels' chunk length
        (grace_topk_segmented_chunk_bf16).  Everything else is the parent's own: offsets, the
        small / large split, the finalize workgroups, the carry layout, and the workspace, whose
        layout does not depend on the element type and whose counters every step's prep launch
        re-zeroes -- the f32 and the bf16 step of one entry run on the same stream, one after the
        other, so they share it.  Kept inside the parent's table entry, so it lives and dies with it."""
        T = self.tables(sizes, device, has_res, dense_out)
        hit = T.get("bf16")
        if hit is not None:
            return hit
        chunk = int(_lib.query("grace_topk_segmented_chunk_bf16", 1 if has_res else 0, 1 if dense_out else 0))
        seg = T["seg_off"].tolist()                      # once per table
        chk, chunk_li = [0], []
        for li, i in enumerate(T["large"].tolist()[:T["n_large"]]):
            c = (seg[i + 1] - seg[i] + chunk - 1) // chunk
            chk.append(chk[-1] + c)
            chunk_li += [li] * c
        hit = dict(T)
        hit["chk_off"] = torch.tensor(chk, dtype=torch.int64).to(device)
        hit["chunk_li"] = torch.tensor(chunk_li or [0], dtype=torch.int32).to(device)
        hit["nchunks"] = chk[-1]
        # the table arguments of grace_topk_segmented_step[_bf16], in the C signature's order
        hit["args"] = (hit["seg_off"].data_ptr(), hit["k_off"].data_ptr(), hit["large"].data_ptr(), hit["n_large"],
                       hit["small"].data_ptr(), hit["n_small"], hit["chk_off"].data_ptr(), hit["chunk_li"].data_ptr(),
                       hit["nchunks"], hit["ws_off"].data_ptr(), hit["fin_off"].data_ptr(), hit["fin_li"].data_ptr(),
                       hit["nfin"], hit["n"])
        T["bf16"] = hit
        return hit

    def local_step(self, flat, sizes, name="bucket", dense=None):
        """The parent's local_step for a float32 or bfloat16 flat gradient; `dense` (world 1; may be
        ``flat`` itself) has the gradient's dtype."""
        g = ops.dev_grad(flat)
        if dense is not None and dense.dtype != g.dtype:
            raise TypeError(f"grace_amd: the dense result of a {g.dtype} gradient must be {g.dtype}, got {dense.dtype}")
        if g.dtype != BF16:
            return super().local_step(flat, sizes, name, dense)
        n = g.numel()
        total, sizes = self._norm_sizes(sizes)
        if total != n:
            raise ValueError("segment sizes do not add up to the buffer")
        res = self.residuals.get(name)
        # always f32, never empty_like(g): the name keeps it if its gradient changes dtype (no contiguity
        # test, as in the parent's rule: ops._f32_residual would restart a name the parent's rule keeps)
        has = res is not None and res.dtype == torch.float32 and res.numel() == n and res.device == g.device
        if not has:
            res = torch.empty(n, dtype=torch.float32, device=g.device)
            self.residuals[name] = res
        T = self.tables_bf16(sizes, g.device, has, dense is not None)
        k_total = T["k_total"]
        pay = torch.empty(2 * k_total, dtype=torch.float32, device=g.device)
        vals, idx = pay[:k_total], pay[k_total:].view(torch.int32)
        carry, valid = self._carry_for(name, res, has, T) if self._use_carry else (None, False)
        _lib.call("grace_topk_segmented_step_bf16", g.data_ptr(), res.data_ptr(), 1 if has else 0, self.beta,
                  self.gamma, *T["args"], vals.data_ptr(), idx.data_ptr(),
                  dense.data_ptr() if dense is not None else None,
                  carry.data_ptr() if carry is not None else None, T["carry_off"].data_ptr(), 1 if valid else 0,
                  T["ws"].data_ptr(), T["ws"].numel(), T["ws_need"], ops._stream())
        if carry is not None:
            self._carries[name] = (carry, res, res._version, T["carry_key"])
        self.last_payload = (vals, idx)
        return pay

    def step(self, flat, sizes, name="bucket", out=None):
        """flat: f32 or bf16 [sum(sizes)] gradients; returns the flat aggregated result in the same
        dtype (``out`` if given, which may be ``flat`` itself)."""
        g = ops.dev_grad(flat)
        if out is not None and out.dtype != g.dtype:
            raise TypeError(f"grace_amd: the result of a {g.dtype} gradient must be {g.dtype}, got {out.dtype}")
        if g.dtype != BF16:
            return super().step(flat, sizes, name, out)
        n = g.numel()
        # refused before anything is stepped: a bad buffer must not cost the name a residual update
        if out is not None and not (out.numel() == n and out.is_contiguous() and out.device == g.device):
            raise ValueError(f"grace_amd: the result buffer must be a contiguous tensor of {n} elements on {g.device}")
        W = int(self.world_size)
        if W == 1:
            dense = out if out is not None else torch.empty_like(g)
            self.local_step(flat, sizes, name, dense)
            return dense
        pay = self.local_step(flat, sizes, name, None)
        # grouped by output chunk, one all-gather, and the decode that rounds ((0 + d_0) + d_1 + ...) / W
        # once to bf16 and writes every element of `out`
        return exchange_decode_sorted(pay, pay.numel() // 2, n, W, W if self.average else 1, out)
