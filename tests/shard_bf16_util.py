"""One process plays all W ranks of the sharded top-k step on one device (test infrastructure for
tests/test_gpu_sharded_bf16.py): every rank's local swap step writes its slot of ONE records buffer
(what the all-gather would deliver), then ops.shard_select runs for each rank over all of them."""
import numpy as np
import torch

from grace_amd import ops

BF16 = torch.bfloat16
CANARY = 0x7FC1      # a bf16 NaN no kernel here produces (f32_to_bf16 makes 0x7FC0)


def bits16(x):
    """the 16-bit patterns of a bf16 tensor, as int32 (0 .. 65535) on the CPU"""
    return x.detach().cpu().contiguous().view(torch.int16).to(torch.int32) & 0xFFFF


def from_bits16(bits, device):
    return torch.tensor(bits, dtype=torch.int32).to(torch.int16).view(BF16).to(device)


class Ranks:
    """The partition `sizes` of one bucket, its k and the gathered-records buffer."""

    def __init__(self, sizes, k, dev, cap=None):
        self.sizes = list(sizes)
        self.world = len(sizes)
        self.n = sum(sizes)
        self.bases = [sum(sizes[:r]) for r in range(self.world)]
        self.k = k
        self.cap = k if cap is None else cap
        self.dev = dev
        self.stride = ops.shard_record_words(self.cap)
        self.tab = torch.tensor(self.sizes + self.bases, dtype=torch.int64, device=dev)
        self.recs = torch.full((self.world * self.stride,), -1, dtype=torch.int32, device=dev)
        for r in range(self.world):
            self.recs[r * self.stride] = self.sizes[r]
            self.recs[r * self.stride + 1:r * self.stride + ops.SHARD_HDR] = 0
        self.status = ops.new_status_word()

    def slot(self, r):
        """(vals f32[cap], idx i32[cap]) views of rank r's record"""
        o = r * self.stride + ops.SHARD_HDR
        return self.recs[o:o + self.cap].view(torch.float32), self.recs[o + self.cap:o + 2 * self.cap]

    def local(self, bucket, res=None):
        """Every rank's local step on its slice of `bucket` (f32 or bf16) with residuals `res` (or
        none): the records are written, the new residuals returned."""
        new = []
        for r in range(self.world):
            vals, idx = self.slot(r)
            out = torch.empty(self.sizes[r], dtype=torch.float32, device=self.dev)
            ops.topk_residual_step_swap(bucket[self.bases[r]:self.bases[r] + self.sizes[r]],
                                        res[r] if res is not None else None, res is not None, 1.0, 1.0,
                                        min(self.cap, self.sizes[r]), out, payload=(None, vals, idx))
            new.append(out)
        return new

    def set_records(self, vals_u32, li, hdr=None):
        """Hand-built records (tests/shard_select_util.py): value bits uint32[W, cap] and local
        indices int32[W, cap] as numpy arrays; header word 0 of rank w = hdr[w] (default its shard
        length), the other header words 0."""
        rec = np.zeros((self.world, self.stride), dtype=np.int32)
        rec[:, 0] = self.sizes if hdr is None else hdr
        rec[:, ops.SHARD_HDR:ops.SHARD_HDR + self.cap] = np.ascontiguousarray(vals_u32, dtype=np.uint32).view(np.int32)
        rec[:, ops.SHARD_HDR + self.cap:] = li
        self.recs.copy_(torch.from_numpy(rec).view(-1))

    def select(self, res, outs, out_base=None, k=None, ranks=None, sel_gi=True):
        """ops.shard_select for every rank (or for `ranks`) into outs[r] (pre-filled by the caller;
        out_base[r] = the global index of its first element, 0 when None), on COPIES of the
        residuals `res` (explicit tensors per rank: a list, or a dict by rank), with this
        partition's k or the call's own; sel_gi=False passes no selection list.
        Returns (the residual copies, pay_idx, sel_gi or None), one entry per rank run, in order."""
        rs, pays, sels = [], [], []
        for r in range(self.world) if ranks is None else ranks:
            rr = res[r].clone()
            pay = torch.full((self.cap,), -1, dtype=torch.int32, device=self.dev)
            sel = torch.full((self.world * self.cap,), -2, dtype=torch.int32, device=self.dev) if sel_gi else None
            ops.shard_select(self.recs, self.world, r, self.cap, self.tab, self.k if k is None else k, rr, outs[r],
                             0 if out_base is None else out_base[r], pay, self.status, sel)
            rs.append(rr)
            pays.append(pay)
            sels.append(sel)
        return rs, pays, sels


def same_i32(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))
