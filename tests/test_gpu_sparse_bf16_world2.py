"""Threshold and random-k on bfloat16 gradients at world size 2 on one GPU (two processes share cuda:0
over gloo, as tests/test_gpu_dgc_bf16_world2.py), through ``Allgather(grace_amd.sparse_bf16.<class>,
memory, 2).step``.  The gradients are tests/test_gpu_world2.py's capacity-exchange threshold gradients
(n = 5003, a 3x tail on rank 1 at step 2) rounded to bf16.

Expected values are the oracle's compensate, select, decode, rank-ordered sum and division on the
widened gradients in f32, with threshold.py's capacity policy restated, then one rounding to bf16
(tests/shard_select_util.round_cpu): ``out`` (bf16) and the residual (f32) are bit-exact on both ranks,
``overflows`` and the capacities are the restated policy's.  Two more threshold runs step the name bf16
on rank 0 and f32 on rank 1: the wire is the same f32 wire, so each rank gets the oracle's sum in its own
dtype.  One pair of processes runs every configuration; the tests below each check their part."""
import os
import tempfile

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from oracle import grace_oracle as O
from tests.golden_util import same_bits
from tests.sparse_bf16_util import BETA, GAMMA, W2_N as N
from tests.sparse_bf16_util import want_bits, world2_thr_grad

pytestmark = pytest.mark.gpu
F32 = np.float32
BF16 = torch.bfloat16
W, THR, THR_STEPS, RK_STEPS, RK_RATIO = 2, 1.5, 4, 3, 0.3
# (key, exchange, margin, overflow, memory, dtypes of rank 0 and rank 1)
THR_RUNS = [
    ("counts", "counts", 1.25, "retry", "residual", (BF16, BF16)),
    ("retry", "capacity", 1.0, "retry", "residual", (BF16, BF16)),
    ("defer", "capacity", 1.0, "defer", "residual", (BF16, BF16)),
    ("none", "counts", 1.25, "retry", "none", (BF16, BF16)),
    ("mixed_counts", "counts", 1.25, "retry", "residual", (BF16, torch.float32)),
    ("mixed_retry", "capacity", 1.0, "retry", "residual", (BF16, torch.float32)),
]


def _save(out):
    return out.view(torch.int16).cpu().numpy() if out.dtype == BF16 else out.cpu().numpy()


def _worker(rank, path, outdir):
    dist.init_process_group("gloo", init_method=f"file://{path}", rank=rank, world_size=W)
    torch.cuda.set_device(0)
    from grace_amd.dist.communicator.allgather import Allgather
    from grace_amd.dist.memory.none import NoneMemory
    from grace_amd.dist.memory.residual import ResidualMemory
    from grace_amd.sparse_bf16 import RandomKCompressor, ThresholdCompressor
    res = {}
    for key, exchange, margin, overflow, memory, dtypes in THR_RUNS:
        comp = ThresholdCompressor(THR, exchange=exchange, capacity_margin=margin, overflow=overflow)
        comm = Allgather(comp, ResidualMemory(BETA, GAMMA) if memory == "residual" else NoneMemory(), W)
        for s in range(THR_STEPS):
            g = torch.from_numpy(world2_thr_grad("cap", rank, s)).cuda()     # bf16 values held in f32: the cast is exact
            out = comm.step(g.to(dtypes[rank]), "thr")
            assert out.dtype == dtypes[rank] and out.shape == g.shape
            res[f"{key}_out{s}"] = _save(out)
            if memory == "residual":
                res[f"{key}_r{s}"] = comm.memory.residuals["thr"].cpu().numpy()
            res[f"{key}_cap{s}"] = np.array([comp.capacity.get("thr", -1)])
        res[f"{key}_overflows"] = np.array([comp.overflows])
    comm = Allgather(RandomKCompressor(RK_RATIO, rng="torch_cpu"), ResidualMemory(BETA, GAMMA), W)
    for s in range(RK_STEPS):
        g = torch.from_numpy(world2_thr_grad("thr", rank, s)).cuda()
        out = comm.step(g.to(BF16), "w")
        assert out.dtype == BF16 and out.shape == g.shape
        res[f"rk_out{s}"] = _save(out)
        res[f"rk_r{s}"] = comm.memory.residuals["w"].cpu().numpy()
    res["rk_global_step"] = np.array([comm.compressor.global_step])
    np.savez(os.path.join(outdir, f"r{rank}.npz"), **res)
    dist.destroy_process_group()


@pytest.fixture(scope="module")
def got():
    with tempfile.TemporaryDirectory() as tmp:
        mp.spawn(_worker, args=(os.path.join(tmp, "rdv"), tmp), nprocs=W, join=True)
        return [dict(np.load(os.path.join(tmp, f"r{r}.npz"))) for r in range(W)]


def _grow(mx, margin):
    return int(min(N, max(64, int(np.ceil(mx * margin)))))


def expected_threshold(exchange, margin, overflow, memory):
    """The reference's steps on the widened gradients with the capacity policy of
    grace_amd/dist/compressor/threshold.py restated -> (per step: out f32, residuals, max count, cap),
    overflows, the steps whose max count was above the capacity they ran with."""
    residual = memory == "residual"
    defer = overflow == "defer" and residual
    state = [None] * W
    cap, pending, overflows, over_steps = None, None, 0, []
    steps = []
    for s in range(THR_STEPS):
        sel = []
        for r in range(W):
            g = world2_thr_grad("cap", r, s)
            t = O.residual_compensate(g, state[r], BETA, GAMMA).ravel() if residual else g
            vals, idx = O.threshold_select(t, THR)
            sel.append((t, vals, idx))
        mx = max(v.size for _, v, _ in sel)
        if defer and pending is not None:
            pmx, pover = pending
            pending = None
            if pover:
                overflows += 1
            if cap is not None and (pover or _grow(pmx, margin) * 4 < cap):
                cap = _grow(pmx, margin)
        send = None                                         # everything travels
        if exchange == "capacity":
            if cap is None or cap > N:
                cap = _grow(mx, margin)
            elif defer:
                send = cap
                pending = (mx, mx > cap)
                over_steps += [s] if mx > cap else []
            elif mx > cap:
                overflows += 1
                over_steps.append(s)
                cap = _grow(mx, margin)
            elif _grow(mx, margin) * 4 < cap:
                cap = _grow(mx, margin)
        decs = []
        for r in range(W):
            t, vals, idx = sel[r]
            if send is not None:
                vals, idx = vals[:send], idx[:send]
            d = O.sparse_decode(vals, idx, N)
            decs.append(d)
            if residual:
                state[r] = O.residual_update(t, d)
        out = (O.python_sum(decs) / F32(W)).astype(F32)
        steps.append((out, list(state), mx, cap))
    return steps, overflows, over_steps


def _check_out(got_r, key, s, want, dtype):
    if dtype == BF16:
        assert np.array_equal(got_r[f"{key}_out{s}"].view(np.uint16).astype(np.int32), want_bits(want)), (key, s)
    else:
        assert same_bits(got_r[f"{key}_out{s}"], want), (key, s)


@pytest.mark.parametrize("run", THR_RUNS, ids=[r[0] for r in THR_RUNS])
def test_threshold_bf16_world2(got, run):
    key, exchange, margin, overflow, memory, dtypes = run
    steps, overflows, _ = expected_threshold(exchange, margin, overflow, memory)
    for s, (out, rs, mx, cap) in enumerate(steps):
        for r in range(W):
            _check_out(got[r], key, s, out, dtypes[r])
            if memory == "residual":
                assert same_bits(got[r][f"{key}_r{s}"], rs[r]), (key, s, r, mx, cap)
            if exchange == "capacity":
                assert int(got[r][f"{key}_cap{s}"][0]) == cap, (key, s, r)
    for r in range(W):
        assert int(got[r][f"{key}_overflows"][0]) == overflows, key
    if exchange == "capacity":
        # as tests/test_gpu_world2.py asserts of the f32 class: the 3x tail overflows the capacity, and
        # every rank takes the same decisions (the deferred run sees it when it settles, a step later)
        assert overflows >= 1


def test_randomk_bf16_world2(got):
    state = [None] * W
    for s in range(RK_STEPS):
        idx = O.randomk_indices("w", s, N, RK_RATIO)[0]
        assert np.unique(idx).size < idx.size
        decs = []
        for r in range(W):
            t = O.residual_compensate(world2_thr_grad("thr", r, s), state[r], BETA, GAMMA).ravel()
            d = O.randomk_decode(t[idx], idx, N)
            state[r] = O.residual_update(t, d)
            decs.append(d)
        out = (O.python_sum(decs) / F32(W)).astype(F32)
        for r in range(W):
            _check_out(got[r], "rk", s, out, BF16)
            assert same_bits(got[r][f"rk_r{s}"], state[r]), (s, r)
    assert int(got[0]["rk_global_step"][0]) == int(got[1]["rk_global_step"][0]) == RK_STEPS
