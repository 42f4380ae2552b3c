"""DGC on bfloat16 gradients at world size 2 on one GPU (two processes share cuda:0 over gloo), through
``Allgather(grace_amd.dgc_bf16.DgcCompressor, DgcMemory, 2).step`` in the four exchange modes of
tests/test_gpu_dgc_world2.py, whose gradients (rounded to bf16), sampling stream, step count and
heavier tail on rank 1 at step 3 these are.

Expected values are that file's ``_expected`` logic restated on the widened gradients: the oracle's
compensate, compress, decode, rank-ordered sum and division in f32, then one rounding to bf16
(tests/shard_select_util.round_cpu).  ``out`` (bf16), ``r`` and ``a`` (f32) are bit-exact on both
ranks; ``overflows``, ``host_reads`` and the capacities are the f32 file's assertions (that the
margin-1.0 runs still overflow on the rounded gradients is checked on the CPU in
tests/test_abi_dgc_bf16.py).  One more run steps the name bf16 on rank 0 and f32 on rank 1: the
records on the wire are the same f32 records, so each rank gets the oracle's sum in its own dtype.
"""
import os
import tempfile

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from oracle import grace_oracle as O
from tests.dgc_bf16_util import W2_N as N
from tests.dgc_bf16_util import world2_grad as _grad
from tests.golden_util import same_bits
from tests.shard_select_util import round_cpu

pytestmark = pytest.mark.gpu
F32 = np.float32
RATIO, MOM, STEPS, W = 0.01, 0.9, 6, 2
MODES = [("counts", 1.25, "defer"), ("capacity", 1.0, "retry"), ("capacity", 1.0, "defer"), ("capacity", 1.5, "defer")]


def _worker(rank, path, outdir, mode, dtypes):
    dist.init_process_group("gloo", init_method=f"file://{path}", rank=rank, world_size=W)
    torch.cuda.set_device(0)
    from grace_amd.dgc_bf16 import DgcCompressor
    from grace_amd.dist.communicator.allgather import Allgather
    from grace_amd.dist.memory.dgc import DgcMemory
    exchange, margin, overflow = mode
    torch.manual_seed(1000 + rank)
    comp = DgcCompressor(RATIO, rng="torch_cpu", exchange=exchange, capacity_margin=margin, overflow=overflow)
    comm = Allgather(comp, DgcMemory(MOM, False, W), W)
    res = {}
    for s in range(STEPS):
        g = torch.from_numpy(_grad(rank, s)).cuda()                 # bf16 values held in f32: the cast is exact
        out = comm.step(g.to(dtypes[rank]), "w")
        assert out.dtype == dtypes[rank] and out.shape == g.shape
        res[f"out{s}"] = out.view(torch.int16).cpu().numpy() if out.dtype == torch.bfloat16 else out.cpu().numpy()
        res[f"r{s}"] = comm.memory.residuals["w"].cpu().numpy()
        res[f"a{s}"] = comm.memory.gradients["w"].cpu().numpy()
        res[f"cap{s}"] = np.array([comp.capacity.get("w", -1)])
    res["overflows"] = np.array([comp.overflows])
    res["host_reads"] = np.array([comp.host_reads])
    np.savez(os.path.join(outdir, f"r{rank}.npz"), **res)
    dist.destroy_process_group()


def _grow(mx, margin):
    return int(min(N, max(64, int(np.ceil(mx * margin)))))


def _expected(mode):
    """The reference's step on the widened gradients, with the capacity policy of dgc.py restated
    (tests/test_gpu_dgc_world2.py's _expected); out is the f32 result, rounded by the caller."""
    exchange, margin, overflow = mode
    gens = [torch.Generator().manual_seed(1000 + r) for r in range(W)]
    ns = max(1, int(N * 0.01))
    state = [(None, None) for _ in range(W)]
    cap, pending, overflows = None, None, 0
    steps = []
    for s in range(STEPS):
        sel = []
        for r in range(W):
            res, acc = state[r]
            t, res, acc = O.dgc_memory_compensate(_grad(r, s), res, acc, MOM)
            sidx = torch.empty([ns]).uniform_(0, N, generator=gens[r]).type(torch.long).numpy()
            vals, idx, _, _ = O.dgc_compress(t, sidx, RATIO)
            sel.append((vals, idx, res, acc))
        mx = max(v.size for v, _, _, _ in sel)
        if exchange == "capacity" and overflow == "defer" and pending is not None:
            pmx, pover = pending
            if pover:
                overflows += 1
            if pover or _grow(pmx, margin) * 4 < cap:
                cap = _grow(pmx, margin)
        if exchange == "counts" or cap is None:
            send = None                                     # everything travels
            if exchange == "capacity":
                cap = _grow(mx, margin)
        elif overflow == "retry":
            send = None
            if mx > cap:
                overflows += 1
                cap = _grow(mx, margin)
            elif _grow(mx, margin) * 4 < cap:
                cap = _grow(mx, margin)
        else:
            send = cap
            pending = (mx, mx > cap)
        decs = []
        for r in range(W):
            vals, idx, res, acc = sel[r]
            if send is not None:
                vals, idx = vals[:send], idx[:send]
            decs.append(O.sparse_decode(vals, idx, N))
            keep = np.ones(N, dtype=bool)
            keep[idx] = False                               # zeroed only where an entry travelled
            state[r] = O.dgc_memory_update(res, acc, ~keep)
        out = (O.python_sum(decs) / F32(W)).astype(F32)
        steps.append((out, [st[0] for st in state], [st[1] for st in state], mx, cap))
    return steps, overflows


def _bf16_bits(out32):
    return round_cpu(torch.from_numpy(out32)).numpy().astype(np.uint16).view(np.int16)


def _run(mode, dtypes):
    with tempfile.TemporaryDirectory() as tmp:
        mp.spawn(_worker, args=(os.path.join(tmp, "rdv"), tmp, mode, dtypes), nprocs=W, join=True)
        return [dict(np.load(os.path.join(tmp, f"r{r}.npz"))) for r in range(W)]


def _check(got, mode, dtypes):
    steps, overflows = _expected(mode)
    for s, (out, rs, accs, mx, cap) in enumerate(steps):
        for r in range(W):
            if dtypes[r] == torch.bfloat16:
                assert np.array_equal(got[r][f"out{s}"], _bf16_bits(out)), (mode, s, r, mx, cap)
            else:
                assert same_bits(got[r][f"out{s}"], out), (mode, s, r, mx, cap)
            assert same_bits(got[r][f"r{s}"], rs[r]), (mode, s, r)
            assert same_bits(got[r][f"a{s}"], accs[r]), (mode, s, r)
            if mode[0] == "capacity":
                assert int(got[r][f"cap{s}"][0]) == cap, (mode, s, r)
    for r in range(W):
        assert int(got[r]["overflows"][0]) == overflows, (mode, [int(g["overflows"][0]) for g in got], overflows)
    return overflows


@pytest.mark.parametrize("mode", MODES)
def test_dgc_bf16_world2_exchange_modes(mode):
    dtypes = (torch.bfloat16, torch.bfloat16)
    got = _run(mode, dtypes)
    overflows = _check(got, mode, dtypes)
    if mode[0] == "counts":
        assert int(got[0]["host_reads"][0]) == STEPS              # one read per step (the W counts)
    elif mode[2] == "defer":
        assert int(got[0]["host_reads"][0]) == 1                  # only the name's first step reads
    if mode == ("capacity", 1.0, "defer") or mode == ("capacity", 1.0, "retry"):
        assert overflows >= 1, "the margin-1.0 run was meant to overflow at least once"


def test_dgc_world2_bf16_and_f32_ranks_share_a_wire():
    mode = ("capacity", 1.0, "retry")
    dtypes = (torch.bfloat16, torch.float32)
    _check(_run(mode, dtypes), mode, dtypes)
