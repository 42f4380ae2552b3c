"""Threshold on bfloat16 gradients at world size 1 (grace_amd.sparse_bf16.ThresholdCompressor,
grace_threshold_step_w1_bf16 of include/grace_hip_sparse.h) against the oracle on the widened gradient:
``out`` is the f32 result rounded once (tests/shard_select_util.round_cpu), the residual and the
workspace's bound are the f32 step's, everything bit for bit.  Three steps per run with beta, gamma =
0.9, 0.7, so that t is no bf16 number from the second step on; every constructed case is first shown,
on the CPU, to land in the branch it is named for (tests/sparse_bf16_util.thr_check_branch)."""
import numpy as np
import pytest
import torch

from grace_amd import ops
from tests.golden_util import same_bits
from tests.sparse_bf16_util import (BETA, GAMMA, STEPS, THR, THR_CASES, THR_SIZES, bits16, bits32, thr_check_branch,
                                    thr_feasible, thr_grad, thr_of, thr_step, want_bits)

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = np.float32
BF16 = torch.bfloat16


def _np(t):
    return t.detach().cpu().numpy()


def _comm(cls, thr, memory):
    from grace_amd.dist.communicator.allgather import Allgather
    from grace_amd.dist.memory.none import NoneMemory
    from grace_amd.dist.memory.residual import ResidualMemory
    return Allgather(cls(thr), ResidualMemory(BETA, GAMMA) if memory == "residual" else NoneMemory(), 1)


def _classes():
    from grace_amd.dist.compressor.threshold import ThresholdCompressor as Parent
    from grace_amd.sparse_bf16 import ThresholdCompressor
    return ThresholdCompressor, Parent


def _bound_bits():
    ws = ops.workspace("threshold", 1, torch.device(DEV, torch.cuda.current_device()))
    return int(_np(ws[:4].view(torch.int32)).view(np.uint32)[0])


@pytest.mark.parametrize("memory", ["none", "residual"])
@pytest.mark.parametrize("case,n", [(c, n) for c in THR_CASES for n in THR_SIZES if thr_feasible(c, n)])
def test_threshold_bf16_cases_three_steps_vs_oracle(case, n, memory):
    thr = thr_of(case)
    residual = memory == "residual"
    comm = _comm(_classes()[0], thr, memory)
    r = None
    for s in range(STEPS):
        gb, gw = thr_grad(case, n, s)
        e = thr_step(gw, r, thr, residual)
        thr_check_branch(case, n, s, e, thr)
        out = comm.step(gb.to(DEV).view(1, n), "w")
        assert out.dtype == BF16 and out.shape == (1, n)
        assert np.array_equal(bits16(out), want_bits(e["out"])), (case, n, s)
        assert _bound_bits() == bits32(e["bound"]), (case, n, s)
        if residual:
            rd = comm.memory.residuals["w"]
            assert rd.dtype == torch.float32 and rd.shape == (1, n)
            assert same_bits(_np(rd).ravel(), e["r"]), (case, n, s)
            r = e["r"]


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("case", ["holds", "neg_fixup"])
def test_threshold_bf16_misaligned_views_take_the_scalar_path(case, mode):
    """g and out one element into 16-byte aligned buffers (2-byte aligned only), the f32 residual one
    element in too: the scalar loop gives the oracle's bits, as the aligned vector path does."""
    n = 16389
    gb, gw = thr_grad(case, n, 1)
    r0 = np.random.default_rng(5).standard_normal(n).astype(F32) * F32(0.05) if mode == 2 else None
    e = thr_step(gw, r0, THR, residual=mode != 0)
    thr_check_branch(case, n, 0 if mode != 2 else 1, e, THR)
    for off in (1, 0):
        gbuf = torch.empty(n + 8, dtype=BF16, device=DEV)
        obuf = torch.empty(n + 8, dtype=BF16, device=DEV)
        rbuf = torch.empty(n + 8, dtype=torch.float32, device=DEV)
        assert gbuf.data_ptr() % 16 == 0 and obuf.data_ptr() % 16 == 0 and rbuf.data_ptr() % 16 == 0
        g, out, res = gbuf[off:off + n], obuf[off:off + n], rbuf[off:off + n]
        g.copy_(gb)
        if mode == 2:
            res.copy_(torch.from_numpy(r0))
        got = ops.threshold_step_w1(g, res if mode else None, mode, BETA, GAMMA, THR, out=out)
        assert got.data_ptr() == out.data_ptr()
        assert np.array_equal(bits16(out), want_bits(e["out"])), (case, mode, off)
        assert _bound_bits() == bits32(e["bound"])
        if mode:
            assert same_bits(_np(res), e["r"]), (case, mode, off)


def test_threshold_name_stepped_f32_bf16_f32_shares_its_residual():
    """One compressor, one name, stepped f32, bf16, f32: the residual after every step is bit for bit
    that of the parent class stepping the widened gradients in f32, and the bf16 step's result is the
    parent's rounded once."""
    n = 16389
    ours, parent = _comm(_classes()[0], 1.5, "residual"), _comm(_classes()[1], 1.5, "residual")
    for s, dtype in enumerate((torch.float32, BF16, torch.float32)):
        gb, gw = thr_grad("neg_fixup" if s == 1 else "holds", n, s)
        out = ours.step(gb.to(DEV).to(dtype), "w")
        ref = parent.step(torch.from_numpy(gw).to(DEV), "w")
        assert out.dtype == dtype
        if dtype == BF16:
            assert np.array_equal(bits16(out), want_bits(_np(ref)))
        else:
            assert same_bits(_np(out), _np(ref))
        assert same_bits(_np(ours.memory.residuals["w"]), _np(parent.memory.residuals["w"])), s


def test_threshold_capacity_exchange_at_world1_writes_bf16():
    """exchange='capacity' at world 1 goes through the compensate, the parent's count / write and the
    two bf16 decodes (padded on the first step, records after): bit for bit the oracle's."""
    from grace_amd.dist.communicator.allgather import Allgather
    from grace_amd.dist.memory.residual import ResidualMemory
    n = 16389
    comp = _classes()[0](1.5, exchange="capacity", capacity_margin=4.0)
    comm = Allgather(comp, ResidualMemory(BETA, GAMMA), 1)
    r = None
    for s in range(STEPS):
        gb, gw = thr_grad("holds", n, s)
        e = thr_step(gw, r, 1.5)
        out = comm.step(gb.to(DEV), "w")
        assert np.array_equal(bits16(out), want_bits(e["out"])), s
        assert same_bits(_np(comm.memory.residuals["w"]), e["r"]), s
        r = e["r"]
    assert comp.capacity["w"] >= 64 and comp.overflows == 0


def test_threshold_float16_and_the_parent_on_bf16_raise_type_error():
    x = torch.zeros(256, device=DEV)
    for memory in ("none", "residual"):
        with pytest.raises(TypeError):
            _comm(_classes()[0], 1.5, memory).step(x.to(torch.float16), "w")
        with pytest.raises(TypeError):
            _comm(_classes()[1], 1.5, memory).step(x.to(BF16), "w")
    for bad in (torch.float16, torch.float64):
        with pytest.raises(TypeError):
            ops.threshold_step_w1(x.to(bad), None, 0, 1.0, 1.0, 1.5)
        with pytest.raises(TypeError):
            ops.axpby_grad(None, x.to(bad), 1.0, 1.0)
    with pytest.raises(TypeError):
        ops.threshold_step_w1(x.to(BF16), x.to(BF16), 1, 1.0, 1.0, 1.5)      # the residual is f32
    with pytest.raises(ValueError):
        ops.threshold_step_w1(x.to(BF16), None, 3, 1.0, 1.0, 1.5)
