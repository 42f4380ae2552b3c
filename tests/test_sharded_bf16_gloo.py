"""grace_amd.sharded_bf16.ShardedTopK on CPU with gloo, W = 2 and 3: bfloat16 shards, a bfloat16
dense result.

The device calls are tests/test_sharded_gloo.py's oracle-backed emulator with the bf16 pieces added
as the kernels define them: the local step widens the gradient (exactly), the select rounds what it
writes once to bfloat16.  Checked against the single-process oracle top-k + residual step
(TopKCompressor, grace_dl/dist/compressor/topk.py:32-42; ResidualMemory, memory/residual.py:10-20) on
the concatenated, widened bucket: the union of the payloads and every residual shard bit for bit,
the dense result == the oracle's rounded once to bfloat16.  Then float32 shards through the same
class against the parent class, and a resize under check_sizes=True.  The GPU version is
tests/test_gpu_sharded_bf16.py."""
import os
import tempfile

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from oracle import grace_oracle as O
from tests.test_sharded_gloo import OracleShardKernels

BF16 = torch.bfloat16
STEPS = 3


class OracleShardKernelsBf16(OracleShardKernels):
    """The emulator on a bf16 gradient (widened, exact) and into a bf16 dense output (the f32 result
    rounded once to nearest even, what grace_shard_select_bf16 stores)."""

    def local_step(self, g, res, has_res, k_loc, vals, idx, res_out):
        super().local_step(g.float(), res, has_res, k_loc, vals, idx, res_out)

    def select(self, recs, world, rank, cap, tab, k, res, out, out_base, pay_idx, status):
        if out.dtype != BF16:
            return super().select(recs, world, rank, cap, tab, k, res, out, out_base, pay_idx, status)
        wide = out.float()
        super().select(recs, world, rank, cap, tab, k, res, wide, out_base, pay_idx, status)
        out.copy_(wide.to(BF16))


def _bucket(n, seed):
    """bf16 normals and the same values widened"""
    g = torch.from_numpy(np.random.default_rng(seed).standard_normal(n).astype(np.float32)).to(BF16)
    return g, g.float().numpy()


def _bf16_bits(x):
    return torch.as_tensor(x).view(torch.int16).numpy().copy()


def _worker(rank, world, path, outdir, sizes, sizes2, check_sizes):
    dist.init_process_group("gloo", init_method=f"file://{path}", rank=rank, world_size=world)
    from grace_amd.dist.sharded import ShardedTopK as F32ShardedTopK
    from grace_amd.sharded_bf16 import ShardedTopK
    res = {}
    configs = [(0.01, "replicated")] if sizes2 else [(r, d) for r in (0.01, 0.3) for d in ("replicated", "shard")]
    for ratio, dense in configs:
        eng = ShardedTopK(ratio, dense=dense, kernels=OracleShardKernelsBf16(), check_sizes=check_sizes)
        tag = f"{ratio}_{dense}_"
        for s in range(STEPS):
            part = sizes2 if (sizes2 and s >= 1) else sizes
            base = sum(part[:rank])
            g, _ = _bucket(sum(part), 100 + s)
            out = eng.step(g[base:base + part[rank]].clone(), "bucket")
            assert out.dtype == BF16
            v, i = eng.last_payload
            keep = i.numpy() >= 0
            res[tag + f"out{s}"] = _bf16_bits(out)
            res[tag + f"vals{s}"] = v.numpy()[keep].copy()
            res[tag + f"idx{s}"] = i.numpy()[keep].copy()
            res[tag + f"res{s}"] = eng.residuals["bucket"].numpy().copy()
            res[tag + f"rs{s}"] = np.array([eng.resizes])
        eng.check(torch.device("cpu"))
        res[tag + "host_reads"] = np.array([eng.host_reads])
    if not sizes2:
        # float32 shards: the class hands them to its parent
        new = ShardedTopK(0.01, kernels=OracleShardKernelsBf16())
        par = F32ShardedTopK(0.01, kernels=OracleShardKernels())
        same = True
        base = sum(sizes[:rank])
        for s in range(2):
            g = _bucket(sum(sizes), 300 + s)[1] * np.float32(1.2345)      # not bf16-representable
            shard = torch.from_numpy(g[base:base + sizes[rank]].copy())
            a, b = new.step(shard.clone(), "w"), par.step(shard.clone(), "w")
            same &= a.dtype == torch.float32 and torch.equal(a.view(torch.int32), b.view(torch.int32))
            same &= torch.equal(new.residuals["w"].view(torch.int32), par.residuals["w"].view(torch.int32))
            same &= all(torch.equal(x.view(torch.int32), y.view(torch.int32))
                        for x, y in zip(new.last_payload, par.last_payload))
        res["f32_same"] = np.array([int(same)])
    np.savez(os.path.join(outdir, f"r{rank}.npz"), **res)
    dist.destroy_process_group()


def _run(sizes, sizes2=None, check_sizes=False):
    world = len(sizes)
    with tempfile.TemporaryDirectory() as tmp:
        mp.spawn(_worker, args=(world, os.path.join(tmp, "rdv"), tmp, sizes, sizes2, check_sizes), nprocs=world,
                 join=True)
        outs = []
        for r in range(world):
            with np.load(os.path.join(tmp, f"r{r}.npz")) as z:
                outs.append({k: z[k] for k in z.files})
    return outs


def _bits(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


def _check_step(outs, tag, s, part, v, i, r_new, out, dense):
    idx = np.concatenate([o[tag + f"idx{s}"] for o in outs]).astype(np.int64)
    vals = np.concatenate([o[tag + f"vals{s}"] for o in outs])
    order = np.argsort(idx)
    assert np.array_equal(idx[order], i.astype(np.int64)), (tag, s)
    assert _bits(vals[order], v), (tag, s)
    assert _bits(np.concatenate([o[tag + f"res{s}"] for o in outs]), r_new), (tag, s)
    want = _bf16_bits(torch.from_numpy(out).to(BF16))
    if dense == "shard":
        assert [o[tag + f"out{s}"].size for o in outs] == list(part)
        assert np.array_equal(np.concatenate([o[tag + f"out{s}"] for o in outs]), want), (tag, s)
    else:
        for o in outs:
            assert np.array_equal(o[tag + f"out{s}"], want), (tag, s)


@pytest.mark.parametrize("sizes", [[5000, 3001], [3001, 17, 4000]])   # 17 < k: the record's padding entries
def test_sharded_bf16_matches_single_bucket(sizes):
    outs = _run(sizes)
    n = sum(sizes)
    for ratio in (0.01, 0.3):
        assert len(sizes) == 2 or O.ratio_k(n, ratio) > 17
        for dense in ("replicated", "shard"):
            tag = f"{ratio}_{dense}_"
            r = None
            rounded = 0
            for s in range(STEPS):
                _, v, i, r, out = O.topk_residual_step(_bucket(n, 100 + s)[1], r, ratio)
                _check_step(outs, tag, s, sizes, v, i, r, out, dense)
                rounded += int((torch.from_numpy(out).to(BF16).float().numpy() != out).sum())
            assert rounded > 0     # from step 1 on t = r + g has low bits: the rounding is exercised
            assert all(int(o[tag + "host_reads"][0]) == 1 for o in outs)
    assert all(int(o["f32_same"][0]) == 1 for o in outs)


def test_sharded_bf16_resize_replans_as_the_parent():
    """check_sizes=True, rank 1's shard shrinks at step 1: every rank re-plans in that step, rank 0
    keeps its error feedback, rank 1 starts from t = g, and the event is counted once."""
    sizes, sizes2 = [5000, 3001], [5000, 2000]
    outs = _run(sizes, sizes2=sizes2, check_sizes=True)
    tag = "0.01_replicated_"
    _, v, i, r, out = O.topk_residual_step(_bucket(sum(sizes), 100)[1], None, 0.01)
    _check_step(outs, tag, 0, sizes, v, i, r, out, "replicated")
    r = np.concatenate([r[:5000], np.zeros(2000, np.float32)])
    for s in (1, 2):
        _, v, i, r, out = O.topk_residual_step(_bucket(sum(sizes2), 100 + s)[1], r, 0.01)
        _check_step(outs, tag, s, sizes2, v, i, r, out, "replicated")
    for o in outs:
        assert [int(o[tag + f"rs{s}"][0]) for s in range(STEPS)] == [0, 1, 1]
