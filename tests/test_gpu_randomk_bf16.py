"""Random-k on bfloat16 gradients at world size 1 (grace_amd.sparse_bf16.RandomKCompressor,
grace_randomk_step_w1_dense_bf16 of include/grace_hip_sparse.h) against the oracle on the widened
gradient: ``out`` is the f32 result rounded once, the residual is the f32 step's, bit for bit.  The
indices are the parent's: torch's CPU stream replayed (``rng="torch_cpu"``), or the device generator's
read back with the seed the class derives.  Three steps with beta, gamma = 0.9, 0.7."""
import numpy as np
import pytest
import torch

from grace_amd import ops
from oracle import grace_oracle as O
from tests.dgc_bf16_util import bf16_pair
from tests.golden_util import same_bits
from tests.sparse_bf16_util import BETA, GAMMA, STEPS, bits16, want_bits

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = np.float32
BF16 = torch.bfloat16
# 1 and 7: the scalar loop; 8192: one whole chunk (the vector path); 8197: a tail chunk; 40000: five chunks
SIZES = [1, 7, 8192, 8197, 40000]


def _np(t):
    return t.detach().cpu().numpy()


def _grad(n, seed):
    """Gaussian with -0, bf16 subnormals, +-inf and NaN at fixed places, rounded to bf16."""
    x = np.random.default_rng(seed).standard_normal(n).astype(F32)
    if n >= 7:
        x[2], x[4], x[5] = -0.0, F32(3e-39), F32(-9.2e-41)
    if n >= 8192:
        x[100], x[2049], x[8191], x[n - 1] = np.inf, -np.inf, np.nan, -0.0
    return bf16_pair(x)


def _comm(cls, ratio, rng, memory="residual"):
    from grace_amd.dist.communicator.allgather import Allgather
    from grace_amd.dist.memory.none import NoneMemory
    from grace_amd.dist.memory.residual import ResidualMemory
    return Allgather(cls(ratio, rng=rng), ResidualMemory(BETA, GAMMA) if memory == "residual" else NoneMemory(), 1)


def _classes():
    from grace_amd.dist.compressor.randomk import RandomKCompressor as Parent
    from grace_amd.sparse_bf16 import RandomKCompressor
    return RandomKCompressor, Parent


def _indices(rng, name, s, n, ratio):
    """What RandomKCompressor._indices draws at its step s for this name."""
    if rng == "torch_cpu":
        return O.randomk_indices(name, s, n, ratio)[0]
    h = sum(bytes(name, encoding="utf8"), s)
    return _np(ops.randomk_indices(h, n, O.ratio_k(n, ratio), torch.device(DEV, torch.cuda.current_device())))


def _oracle_step(gw, r, idx):
    with np.errstate(invalid="ignore", over="ignore"):
        t = O.residual_compensate(gw, r, BETA, GAMMA).ravel()
        dec = O.randomk_decode(t[idx], idx, t.size)
        return (O.python_sum([dec]) / F32(1)).astype(F32), O.residual_update(t, dec)


@pytest.mark.parametrize("rng", ["torch_cpu", "device"])
@pytest.mark.parametrize("ratio", [0.01, 0.5])
@pytest.mark.parametrize("n", SIZES)
def test_randomk_bf16_three_steps_vs_oracle(n, ratio, rng):
    """The first step (no residual) and two has_residual steps."""
    comm = _comm(_classes()[0], ratio, rng)
    r = None
    for s in range(STEPS):
        gb, gw = _grad(n, 31 * n + s)
        idx = _indices(rng, "w", s, n, ratio)
        assert idx.size == max(1, int(n * ratio))
        if ratio == 0.5 and n >= 8192:
            assert np.unique(idx).size < idx.size, "the draw was meant to contain duplicates"
        want_out, want_r = _oracle_step(gw, r, idx)
        out = comm.step(gb.to(DEV).view(n, 1), "w")
        assert out.dtype == BF16 and out.shape == (n, 1)
        assert np.array_equal(bits16(out), want_bits(want_out)), (n, ratio, rng, s)
        rd = comm.memory.residuals["w"]
        assert rd.dtype == torch.float32 and same_bits(_np(rd).ravel(), want_r), (n, ratio, rng, s)
        r = want_r
    assert comm.compressor.global_step == STEPS


@pytest.mark.parametrize("has", [False, True])
def test_randomk_bf16_misaligned_views_take_the_scalar_path(has):
    """g and out one element into 16-byte aligned buffers, the residual too: every chunk takes the scalar
    loop and gives the oracle's bits, as the aligned run does."""
    n = 8197 + 8192
    gb, gw = _grad(n, 3)
    r0 = np.random.default_rng(4).standard_normal(n).astype(F32) if has else None
    idx = O.randomk_indices("w", 0, n, 0.5)[0]
    want_out, want_r = _oracle_step(gw, r0, idx)
    for off in (1, 0):
        gbuf = torch.empty(n + 8, dtype=BF16, device=DEV)
        obuf = torch.empty(n + 8, dtype=BF16, device=DEV)
        rbuf = torch.empty(n + 8, dtype=torch.float32, device=DEV)
        assert gbuf.data_ptr() % 16 == 0 and obuf.data_ptr() % 16 == 0 and rbuf.data_ptr() % 16 == 0
        g, out, res = gbuf[off:off + n], obuf[off:off + n], rbuf[off:off + n]
        g.copy_(gb)
        if has:
            res.copy_(torch.from_numpy(r0))
        ops.randomk_step_w1_dense_bf16(g, res, has, BETA, GAMMA, torch.from_numpy(idx).to(DEV), out=out)
        assert np.array_equal(bits16(out), want_bits(want_out)), (has, off)
        assert same_bits(_np(res), want_r), (has, off)


@pytest.mark.parametrize("rng", ["torch_cpu", "device"])
def test_randomk_global_step_sequence_is_shared_by_f32_and_bf16_steps(rng):
    """One instance stepped f32, bf16, f32 draws what the parent draws in three f32 steps on the widened
    gradients: the same counter, the same residual bit for bit, the bf16 result the parent's rounded."""
    n = 8197
    ours, parent = _comm(_classes()[0], 0.5, rng), _comm(_classes()[1], 0.5, rng)
    for s, dtype in enumerate((torch.float32, BF16, torch.float32)):
        gb, gw = _grad(n, 77 + s)
        out = ours.step(gb.to(DEV).to(dtype), "w")
        ref = parent.step(torch.from_numpy(gw).to(DEV), "w")
        assert out.dtype == dtype and ours.compressor.global_step == parent.compressor.global_step == s + 1
        if dtype == BF16:
            assert np.array_equal(bits16(out), want_bits(_np(ref))), s
        else:
            assert same_bits(_np(out), _np(ref)), s
        assert same_bits(_np(ours.memory.residuals["w"]).ravel(), _np(parent.memory.residuals["w"]).ravel()), s


def test_randomk_none_memory_and_float16_raise_type_error():
    x = torch.zeros(256, device=DEV)
    cls = _classes()[0]
    with pytest.raises(TypeError):
        _comm(cls, 0.5, "device", "none").step(x.to(BF16), "w")
    with pytest.raises(TypeError):
        _comm(cls, 0.5, "device", "none").step(x.to(torch.float16), "w")
    with pytest.raises(TypeError):
        _comm(cls, 0.5, "device").step(x.to(torch.float16), "w")
    with pytest.raises(TypeError):
        _comm(_classes()[1], 0.5, "device").step(x.to(BF16), "w")              # the parent is as it was
    idx = torch.zeros(4, dtype=torch.int64, device=DEV)
    with pytest.raises(TypeError):
        ops.randomk_step_w1_dense_bf16(x, x.clone(), False, 1.0, 1.0, idx)        # an f32 gradient
    with pytest.raises(TypeError):
        ops.randomk_step_w1_dense_bf16(x.to(BF16), x.to(BF16), False, 1.0, 1.0, idx)   # the residual is f32
    with pytest.raises(ValueError):
        ops.randomk_step_w1_dense_bf16(x.to(BF16), x.clone(), False, 1.0, 1.0, idx.to(torch.int32))
