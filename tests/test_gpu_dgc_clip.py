"""DGC gradient clipping on the GPU: ``grace_sumsq`` / ``grace_clip_by_sumsq`` (grace_amd/csrc/dgc.hip)
and ``DgcMemory(gradient_clipping=True)``.

The reference's clipping raises (``dist.all_reduce`` returns None, grace_dl/dist/memory/dgc.py:18-19);
the documented intent is ``tensor.clamp(-c, c)`` with ``c = sqrt(all_reduce(sum(g * g)) / world)``,
which the oracle restates as ``O.dgc_clip``.  Parity bar, as for QSGD's "codewords given the norm":
the clip is bit-exact given the sum of squares s (NaN positions by NaN-ness); s itself is within
1 ulp of the exact sum (tests/test_gpu_elementwise.py).  torch.clamp propagates NaN both ways: a NaN
element stays NaN, and a NaN s -- a NaN anywhere in the gradient -- makes every element NaN.

At world 1 the bound is the gradient's own 2-norm, which no finite element exceeds, so the clip bites
only at world > 1 (a rank whose gradient carries more than its share of the summed squares): the
world-2 test plants such a spike on rank 0.
"""
import datetime
import os
import tempfile

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from grace_amd import ops
from oracle import grace_oracle as O
from tests.golden_util import same_bits
from tests.test_gpu_elementwise import Slot, check, close, exact_sums, untouched, values

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = np.float32
T32 = torch.float32


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _np(t):
    return t.detach().cpu().numpy()


def _s(v):
    return torch.tensor([v], dtype=T32, device=DEV)


def _bound(s, world):
    with np.errstate(all="ignore"):
        return np.sqrt(F32(s) / F32(world))


# ----------------------------------------------------------------------------- the kernel, s injected
@pytest.mark.parametrize("off", [False, True], ids=["aligned", "offset"])
@pytest.mark.parametrize("world", [1, 2, 8])
@pytest.mark.parametrize("n", [1, 5, 4099, 1_048_579])
def test_clip_by_sumsq_matches_oracle(n, world, off):
    """Standard normal x with +-0, +-NaN, +-inf and +-1e-45 planted, bounds from well inside the
    data to beyond it; 1,048,579 elements are two grid-stride trips and a ragged end."""
    x0 = values(n, 2)
    x = Slot(n, T32, off, x0)
    for s in (0.02, 0.5, 3.0, float(n)):
        exp = O.dgc_clip(x0, F32(s), world)
        check(ops.clip_by_sumsq(x.t, _s(s), world), exp, s)
        if n >= 4099 and s <= 3.0:
            with np.errstate(all="ignore"):
                assert (np.abs(x0) > _bound(s, world)).sum() > 8, "the bound clips nothing finite"
    untouched(x, x0)


@pytest.mark.parametrize("off", [False, True], ids=["aligned", "offset"])
@pytest.mark.parametrize("n", [5, 4099])
def test_clip_special_values(n, off):
    """The cases with an exact expectation, each also against the oracle."""
    x0 = np.random.default_rng(n).standard_normal(n).astype(F32)
    assert np.all(x0 != 0)
    k = n // 2

    def run(x, s, world=2):
        got = _np(ops.clip_by_sumsq(Slot(n, T32, off, x).t, _s(s), world))
        check(got, O.dgc_clip(x, F32(s), world), s)
        return got

    # a NaN element, finite s: NaN there, the rest clipped
    x = x0.copy()
    x[k] = np.nan
    c = _bound(0.5, 2)
    got = run(x, 0.5)
    assert np.isnan(got[k]) and np.isnan(got).sum() == 1
    rest = np.arange(n) != k
    assert same_bits(got[rest], np.clip(x0, -c, c)[rest]) and np.abs(got[rest]).max() == c
    # NaN s (and a negative one, whose square root is NaN): every element NaN
    assert np.isnan(run(x0, np.nan)).all()
    assert np.isnan(run(x0, -1.0)).all()
    # +inf s: x unchanged
    assert same_bits(run(x0, np.inf), x0)
    # s = 0, non-zero x: zeros that keep the sign of x
    got = run(x0, 0.0)
    assert np.all(got == 0) and np.array_equal(np.signbit(got), np.signbit(x0))
    # +-inf elements: +-c
    x = x0.copy()
    x[0], x[k], x[n - 1] = np.inf, -np.inf, np.inf
    got = run(x, 0.5)
    assert same_bits(got[[0, k, n - 1]], np.array([c, -c, c], dtype=F32))


# ----------------------------------------------------------------------------- DgcMemory, world 1
N1, RATIO, MOM = 100_003, 0.01, 0.9


def _sample_stream(seed, n):
    """The reference's sample indices (compressor/dgc.py:17-19) from a CPU generator seeded like
    torch's global one, which DgcCompressor(rng="torch_cpu") draws from."""
    gen = torch.Generator().manual_seed(seed)
    return torch.empty([max(1, int(n * 0.01))]).uniform_(0, n, generator=gen).type(torch.long).numpy()


def _oracle_step(g_clipped, r, a, sidx, n):
    """memory/dgc.py:21-39 + compressor/dgc.py:12-50 + allgather.py:40-45 at world 1, as
    tests/test_gpu_dgc.py::test_dgc_memory_sequence_golden walks it: (out, r, a)."""
    t, r, a = O.dgc_memory_compensate(g_clipped, r, a, MOM)
    vals, idx, mask, _ = O.dgc_compress(t, sidx, RATIO)
    out = (O.python_sum([O.sparse_decode(vals, idx, n)]) / F32(1)).astype(F32)
    r, a = O.dgc_memory_update(r, a, mask)
    return out, r, a


def _clipping_comm():
    from grace_amd.dist.communicator.allgather import Allgather
    from grace_amd.dist.compressor.dgc import DgcCompressor
    from grace_amd.dist.memory.dgc import DgcMemory
    return Allgather(DgcCompressor(RATIO, rng="torch_cpu"), DgcMemory(MOM, True, 1), 1)


def test_dgc_memory_clipping_sequence():
    """Three steps of Allgather(DgcCompressor, DgcMemory(0.9, True, 1), 1).step: with clipping on the
    step takes the unfused path (compensate, select, one pass for the mask and the output).  The
    kernel is deterministic, so ops.sumsq(g) read back is the s that compensate used; output,
    residual and accumulator bit-exact against the oracle sequence fed O.dgc_clip(g, s, 1)."""
    comm = _clipping_comm()
    r = a = None
    for step in range(3):
        g0 = np.random.default_rng(500 + step).standard_normal(N1).astype(F32)
        g0[[3, N1 // 2, N1 - 1]] = (np.inf if step == 1 else 40.0, -0.0, -25.0)
        g = _t(g0)
        s = _np(ops.sumsq(g))[0]
        if step != 1:
            close(s, F32(exact_sums(g0)["sq"]), 1, f"sumsq step {step} vs exact")
        else:
            assert s == np.inf
        torch.manual_seed(900 + step)
        out = comm.step(g, "w")
        exp, r, a = _oracle_step(O.dgc_clip(g0, s, 1), r, a, _sample_stream(900 + step, N1), N1)
        check(out, exp, ("out", step))
        check(comm.memory.residuals["w"], r, ("residual", step))
        check(comm.memory.gradients["w"], a, ("accumulator", step))
        assert np.count_nonzero(exp) > 0
        assert same_bits(_np(g), g0), "the gradient was modified"


def test_dgc_memory_clipping_nan_gradient():
    """A NaN in g makes s and the bound NaN: the clipped gradient, and so compensate's output, the
    residual and the accumulator, are all NaN, as ``g.clamp(-c, c)`` gives.  The NaN sample threshold
    then selects nothing (compressor/dgc.py:20-36), so the step's result is the oracle's zeros."""
    comm = _clipping_comm()
    g0 = np.random.default_rng(77).standard_normal(N1).astype(F32)
    g0[N1 // 3] = np.nan
    g = _t(g0)
    s = _np(ops.sumsq(g))[0]
    assert np.isnan(s)
    t = comm.memory.compensate(g, "probe")
    assert torch.isnan(t).all() and torch.isnan(comm.memory.residuals["probe"]).all()
    assert torch.isnan(comm.memory.gradients["probe"]).all()
    torch.manual_seed(5)
    out = comm.step(g, "w")
    exp, r, a = _oracle_step(O.dgc_clip(g0, s, 1), None, None, _sample_stream(5, N1), N1)
    assert np.isnan(a).all() and np.isnan(r).all()
    check(out, exp, "out")
    check(comm.memory.residuals["w"], r, "residual")
    check(comm.memory.gradients["w"], a, "accumulator")
    assert same_bits(_np(g), g0), "the gradient was modified"


# ----------------------------------------------------------------------------- DgcMemory, world 2
N2, STEPS2, W = 50_000, 2, 2


def _grad2(rank, step):
    g = np.random.default_rng(6000 + 10 * rank + step).standard_normal(N2).astype(F32)
    if rank == 0:
        g[7 + step] = F32(3000.0)       # more than its share of the summed squares: the clip bites
        g[N2 - 3] = F32(-2500.0)
    return g


def _worker(rank, path, outdir):
    dist.init_process_group("gloo", init_method=f"file://{path}", rank=rank, world_size=W,
                            timeout=datetime.timedelta(seconds=120))
    torch.cuda.set_device(0)
    from grace_amd.dist.memory.dgc import DgcMemory
    try:
        probe = torch.full((1,), float(rank + 1), device="cuda")
        dist.all_reduce(probe)
        refused = None if float(probe.item()) == 3.0 else f"all_reduce gave {float(probe.item())}, not 3"
    except RuntimeError as e:        # the backend has no all-reduce for a GPU tensor
        refused = f"{type(e).__name__}: {e}"
    if refused is not None:
        with open(os.path.join(outdir, f"refused{rank}.txt"), "w") as f:
            f.write(refused)
        dist.destroy_process_group()
        return
    mem = DgcMemory(MOM, True, W)
    res = {}
    for s in range(STEPS2):
        g = torch.from_numpy(_grad2(rank, s)).cuda()
        res[f"s{s}"] = ops.sumsq(g).cpu().numpy()
        t = mem.compensate(g, "w")
        res[f"t{s}"] = t.cpu().numpy()
        res[f"r{s}"] = mem.residuals["w"].cpu().numpy()
        res[f"a{s}"] = mem.gradients["w"].cpu().numpy()
        res[f"g{s}"] = g.cpu().numpy()
    np.savez(os.path.join(outdir, f"r{rank}.npz"), **res)
    dist.destroy_process_group()


def test_dgc_memory_clipping_world2():
    """Two processes on one GPU over gloo: DgcMemory(0.9, True, 2).compensate all-reduces the two
    ranks' sums of squares (the only test of that all-reduce).  Each rank saves its own
    ops.sumsq(g); c = sqrt((s0 + s1) / 2) in f32, and both ranks' accumulator and residual are
    bit-exact against O.dgc_memory_compensate on the clipped gradients.  Skipped, with the backend's
    reason, where gloo refuses an all-reduce on a GPU tensor."""
    with tempfile.TemporaryDirectory() as tmp:
        mp.spawn(_worker, args=(os.path.join(tmp, "rdv"), tmp), nprocs=W, join=True)
        refusals = [open(os.path.join(tmp, f)).read() for f in sorted(os.listdir(tmp)) if f.startswith("refused")]
        if refusals:
            pytest.skip("gloo refused an all-reduce on a GPU tensor: " + refusals[0][:300])
        got = [dict(np.load(os.path.join(tmp, f"r{r}.npz"))) for r in range(W)]
    state = [(None, None)] * W
    for s in range(STEPS2):
        total = F32(F32(got[0][f"s{s}"][0]) + F32(got[1][f"s{s}"][0]))
        for r in range(W):
            g0 = _grad2(r, s)
            close(got[r][f"s{s}"][0], F32(exact_sums(g0)["sq"]), 1, f"sumsq rank {r} step {s} vs exact")
            clipped = O.dgc_clip(g0, total, W)
            if r == 0:
                assert (clipped != g0).sum() >= 1, "the bound clips nothing on rank 0"
            t, res, acc = O.dgc_memory_compensate(clipped, *state[r], MOM)
            state[r] = (res, acc)
            assert same_bits(got[r][f"t{s}"], t), (s, r, "returned accumulator")
            assert same_bits(got[r][f"a{s}"], acc), (s, r, "accumulator")
            assert same_bits(got[r][f"r{s}"], res), (s, r, "residual")
            assert same_bits(got[r][f"g{s}"], g0), (s, r, "the gradient was modified")
