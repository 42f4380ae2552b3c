"""bfloat16 gradients through the HIP top-k engine (grace_amd/csrc/topk.hip, element type uint16_t),
at the level of grace_amd.ops (the C ABI's bf16 entry points) and the Horovod-flavour compress.

The specification: every result is what the f32 path gives for the gradient widened to f32 (exact).
So the expected payload, t and residual come from the oracle on the upcast array, bit for bit, and
the expected dense result is the oracle's f32 result rounded by torch's CPU ``.to(torch.bfloat16)``,
compared as 16-bit patterns (at NaN positions only NaN-ness: the payload bits of a NaN are free).
Inputs are drawn in f32 from a seed and rounded to bf16 by torch on the CPU before use."""
import functools

import numpy as np
import pytest
import torch

from oracle import grace_oracle as O
from tests.golden_util import same_bits

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16 = torch.bfloat16


def _np(t):
    return t.detach().cpu().numpy()


def _inputs_f32(n, kind, seed):
    """The input kinds of tests/test_gpu_topk.py::_inputs."""
    g = np.random.default_rng(seed)
    if kind == "normal":
        return g.standard_normal(n).astype(np.float32)
    if kind == "ties":
        return (np.round(g.standard_normal(n) * 4) / 4).astype(np.float32)
    if kind == "sparse":        # mostly zeros: forces the exact fallback when k > nnz
        x = np.zeros(n, dtype=np.float32)
        pos = g.choice(n, size=max(1, n // 400), replace=False)
        x[pos] = g.standard_normal(pos.size).astype(np.float32)
        return x
    if kind == "special":
        x = g.standard_normal(n).astype(np.float32)
        x[g.choice(n, 5, replace=False)] = np.nan
        x[g.choice(n, 5, replace=False)] = np.inf
        x[g.choice(n, 5, replace=False)] = -np.inf
        x[g.choice(n, 50, replace=False)] = -0.0
        return x
    raise ValueError(kind)


@functools.lru_cache(maxsize=None)
def _inputs(n, kind, seed):
    """(bf16 CPU tensor, its exact f32 upcast as a read-only numpy array)."""
    b = torch.from_numpy(_inputs_f32(n, kind, seed)).to(BF16)
    up = b.float().numpy()
    up.setflags(write=False)
    return b, up


def _bits16(t):
    return t.detach().cpu().contiguous().view(torch.int16).numpy().ravel()


def check_dense(out, exp_f32):
    """out (bf16 tensor) == exp_f32 rounded to bf16 as torch's CPU cast rounds, bit for bit."""
    assert out.dtype == BF16
    exp = torch.from_numpy(np.ascontiguousarray(exp_f32, dtype=np.float32)).to(BF16)
    got_nan, exp_nan = torch.isnan(out.detach().cpu().float()).numpy().ravel(), np.isnan(exp_f32).ravel()
    assert np.array_equal(got_nan, exp_nan), "NaN positions differ"
    ok = ~exp_nan
    assert np.array_equal(_bits16(out)[ok], _bits16(exp)[ok]), "bf16 result bits differ"


def check_topk(x_np, k, vals, idx):
    """tests/test_gpu_topk.py's check: the oracle's index set and payload values, bit for bit."""
    ov, oi = O.topk_select(x_np, k)
    v, i = _np(vals), _np(idx).astype(np.int64)
    o = np.argsort(i, kind="stable")
    v, i = v[o], i[o]
    assert vals.dtype == torch.float32 and idx.dtype == torch.int32
    assert i.size == k
    assert np.array_equal(i, oi.astype(np.int64)), "index set differs from oracle"
    assert same_bits(v, ov), "payload values differ from oracle"


def _oracle_step(up, res, k, beta=1.0, gamma=1.0):
    """(t, new residual, world-1 dense result in f32) of one residual step on the upcast gradient."""
    t = O.residual_compensate(up, res, beta, gamma).ravel()
    vals, idx = O.topk_select(t, k)
    dec = O.sparse_decode(vals, idx, t.size)
    return t, O.residual_update(t, dec), O.python_sum([dec]), dec


# ------------------------------------------------------------------------------- 1. conversion
@functools.lru_cache(maxsize=None)
def _conversion_cases():
    hi = np.arange(65536, dtype=np.uint32) << 16
    lows = np.array([0x0000, 0x0001, 0x7FFF, 0x8000, 0x8001, 0xFFFF], dtype=np.uint32)
    u = (hi[:, None] | lows[None, :]).ravel()
    assert u.size == 393216
    x = torch.from_numpy(u.view(np.float32).copy())
    return x, x.to(BF16)


@pytest.mark.parametrize("case", ["all", "tail3", "offset_out"])
def test_f32_to_bf16_every_rounding_decision(case):
    """Every upper half x every lower half that decides a rounding (ties, just above / below,
    subnormals, +-inf, NaN) against torch's CPU cast; a length with n mod 4 = 3 and an output view
    one element (2 bytes) into its buffer take the guarded path."""
    from grace_amd import ops
    x, exp = _conversion_cases()
    n = x.numel()
    if case == "tail3":
        n -= 1
        assert n % 4 == 3
    xd = x[:n].to(DEV)
    if case == "offset_out":
        buf = torch.zeros(n + 1, dtype=BF16, device=DEV)
        out = ops.f32_to_bf16(xd, out=buf[1:])
        assert out.data_ptr() == buf.data_ptr() + 2 and _bits16(buf[:1])[0] == 0
    else:
        out = ops.f32_to_bf16(xd)
    assert out.dtype == BF16 and out.shape == xd.shape
    nan = torch.isnan(x[:n]).numpy()
    assert np.array_equal(torch.isnan(out.cpu().float()).numpy(), nan)
    assert np.array_equal(_bits16(out)[~nan], _bits16(exp[:n])[~nan])


# ------------------------------------------------------------------------------- 2. compress, NoneMemory
@pytest.mark.parametrize("n", [1000, 32768, 32769, 100003, 1 << 20])
@pytest.mark.parametrize("ratio", [0.01, 0.3])
@pytest.mark.parametrize("kind", ["normal", "ties", "sparse", "special"])
def test_bf16_compress_and_nomemory_step(n, ratio, kind):
    """ops.topk_compress and the one-pass no-memory step ops.topk_step_dense (payload and
    (0 + decode) / 1) on a bf16 tensor, flat or as a column; the input is left untouched."""
    from grace_amd import ops
    b, up = _inputs(n, kind, n + 3)
    xd = b.to(DEV)
    k = O.ratio_k(n, ratio)
    _, vals, idx = ops.topk_compress(xd, k)
    check_topk(up, k, vals, idx)
    expect = np.float32(0.0) + O.sparse_decode(*O.topk_select(up, k), n)     # Python sum starts at 0
    _, vals, idx, out = ops.topk_step_dense(xd, k)
    check_topk(up, k, vals, idx)
    check_dense(out, expect)
    _, cv, ci = ops.topk_compress(xd.view(-1, 1), k)
    check_topk(up, k, cv, ci)
    out2 = torch.empty(n, dtype=BF16, device=DEV)
    assert ops.topk_step_dense(xd.view(-1, 1), k, out=out2)[3] is out2
    check_dense(out2, expect)
    assert np.array_equal(_bits16(xd), _bits16(b)), "the input was modified"


def test_bf16_k_covers_the_bucket():
    """k >= n on a bucket past the single-workgroup size: every element selected (topk_all)."""
    from grace_amd import ops
    n = 40000
    b, up = _inputs(n, "special", 11)
    xd = b.to(DEV)
    _, vals, idx, out = ops.topk_step_dense(xd, n)
    check_topk(up, n, vals, idx)
    check_dense(out, np.float32(0.0) + up)
    _, vals, idx = ops.topk_compress(xd, n)
    check_topk(up, n, vals, idx)


# ------------------------------------------------------------------------------- 3. residual step, world 1
@pytest.mark.parametrize("n", [40000, (1 << 21) + 5])
@pytest.mark.parametrize("beta,gamma", [(1.0, 1.0), (0.9, 0.5)])
@pytest.mark.parametrize("kind", ["normal", "special"])
def test_bf16_residual_step_world1(n, beta, gamma, kind):
    """Three steps on one residual (ops.topk_residual_step with a bf16 result): payload, f32
    residual bits and bf16 result bits after each (the single-workgroup size, once as a 2-D gradient,
    and a many-chunk size with an odd tail; the residual-sample carry starts at 2^24 elements:
    test_bf16_residual_step_carry_live)."""
    from grace_amd import ops
    k = O.ratio_k(n, 0.01)
    shape = (200, 200) if n == 40000 else (n,)
    r = torch.empty(n, dtype=torch.float32, device=DEV)
    res = None
    for s in range(3):
        b, up = _inputs(n, kind, 100 * s + 7)
        gd = b.to(DEV).view(shape)
        out = torch.empty_like(gd)
        _, vals, idx = ops.topk_residual_step(gd, r, s > 0, beta, gamma, k, out=out)
        t, res, exp_out, _ = _oracle_step(up, res, k, beta, gamma)
        assert out.dtype == BF16 and out.shape == gd.shape
        check_topk(t, k, vals, idx)
        assert same_bits(_np(r), res), f"residual differs at step {s}"
        check_dense(out.reshape(-1), exp_out)


@pytest.mark.parametrize("kind,beta,gamma", [("normal", 1.0, 1.0), ("special", 0.9, 0.5)])
def test_bf16_residual_step_carry_live(kind, beta, gamma):
    """The smallest bucket whose bracket keeps a residual-sample carry (stratum 256 at 2^24
    elements): the second step's bracket derives r' at its sample positions from the carry and reads
    only the bf16 gradient there -- once with unit factors, once with beta, gamma != 1 on inputs with
    NaN, +-inf and -0.  Two steps, checked like the three above."""
    from grace_amd import ops
    n = 1 << 24     # 65,536 samples up to here (stratum 256); 131,072 (stratum 128) just above
    k = O.ratio_k(n, 0.01)
    size = ops.topk_carry_size(n, k)
    assert size > 0
    r = torch.empty(n, dtype=torch.float32, device=DEV)
    carry = torch.empty(size, dtype=torch.float32, device=DEV)
    res = None
    for s in range(2):
        b, up = _inputs(n, kind, 300 + s)
        out = torch.empty(n, dtype=BF16, device=DEV)
        _, vals, idx = ops.topk_residual_step(b.to(DEV), r, s > 0, beta, gamma, k, out=out, carry=carry,
                                              carry_valid=s > 0)
        t, res, exp_out, _ = _oracle_step(up, res, k, beta, gamma)
        check_topk(t, k, vals, idx)
        assert same_bits(_np(r), res), f"residual differs at step {s}"
        check_dense(out, exp_out)
    _inputs.cache_clear()   # (the two 2^24-element inputs)


@pytest.mark.parametrize("n", [100003, (1 << 20) + 7])
def test_bf16_residual_step_exact_fallback(n):
    """Mostly-zero gradients (k > non-zeros): both steps take the exact fallback, which must find t
    again after the main pass -- from g on the first step, from r (where the bf16 pass leaves t,
    unlike the f32 pass, which parks it in the f32 dense output) on the second."""
    from grace_amd import ops
    k = O.ratio_k(n, 0.01)
    r = torch.empty(n, dtype=torch.float32, device=DEV)
    res = None
    for s in range(2):
        b, up = _inputs(n, "sparse", 500 + s)
        out = torch.empty(n, dtype=BF16, device=DEV)
        _, vals, idx = ops.topk_residual_step(b.to(DEV), r, s > 0, 1.0, 1.0, k, out=out)
        assert ops.topk_status(n, k, r.device) == 1, "expected the exact fallback"
        t, res, exp_out, _ = _oracle_step(up, res, k)
        check_topk(t, k, vals, idx)
        assert same_bits(_np(r), res), f"residual differs at step {s}"
        check_dense(out, exp_out)


# ------------------------------------------------------------------------------- 4. alignment
def test_bf16_residual_step_unaligned_views():
    """g and the preallocated out one element (2 bytes) into larger bf16 buffers: the guarded path."""
    from grace_amd import ops
    n = 100003
    k = O.ratio_k(n, 0.01)
    r = torch.empty(n, dtype=torch.float32, device=DEV)
    res = None
    for s in range(2):
        b, up = _inputs(n, "normal", 40 + s)
        gbuf = torch.zeros(n + 1, dtype=BF16, device=DEV)
        obuf = torch.zeros(n + 1, dtype=BF16, device=DEV)
        gbuf[1:].copy_(b)
        g, out = gbuf[1:], obuf[1:]
        assert g.data_ptr() % 8 == 2 and out.data_ptr() % 8 == 2
        _, vals, idx = ops.topk_residual_step(g, r, s > 0, 1.0, 1.0, k, out=out)
        t, res, exp_out, _ = _oracle_step(up, res, k)
        check_topk(t, k, vals, idx)
        assert same_bits(_np(r), res)
        check_dense(out, exp_out)
        assert _bits16(obuf[:1])[0] == 0, "wrote before the view"


# ------------------------------------------------------------------------------- 5. world > 1 local steps
@pytest.mark.parametrize("mode", ["swap", "in_place"])
def test_bf16_swap_and_in_place_steps(mode):
    """ops.topk_residual_step_swap and ops.topk_residual_step(out=None) on a bf16 gradient, two
    steps: payload and new residual against the oracle; the swap leaves the old residual alone."""
    from grace_amd import ops
    n = (1 << 20) + 7
    k = O.ratio_k(n, 0.01)
    bufs = [torch.empty(n, dtype=torch.float32, device=DEV) for _ in range(2)]
    res = None
    for s in range(2):
        b, up = _inputs(n, "normal", 60 + s)
        g = b.to(DEV)
        t, new_res, _, _ = _oracle_step(up, res, k)
        if mode == "swap":
            old, new = bufs[(s + 1) % 2], bufs[s % 2]
            before = old.clone() if s else None
            _, vals, idx = ops.topk_residual_step_swap(g, old if s else None, s > 0, 1.0, 1.0, k, new)
            if s:
                assert torch.equal(old.view(torch.int32), before.view(torch.int32)), "old residual modified"
        else:
            new = bufs[0]
            _, vals, idx = ops.topk_residual_step(g, new, s > 0, 1.0, 1.0, k, out=None)
        check_topk(t, k, vals, idx)
        assert same_bits(_np(new), new_res), f"residual differs at step {s}"
        res = new_res


# ------------------------------------------------------------------------------- 6. today's workaround
def test_bf16_step_equals_upcast_step_downcast():
    """The bf16 step against cast up, f32 step, cast down (on the device), bit for bit, residuals
    included."""
    from grace_amd import ops
    n = 1 << 20
    k = O.ratio_k(n, 0.01)
    r, r32 = (torch.empty(n, dtype=torch.float32, device=DEV) for _ in range(2))
    for s in range(2):
        g = _inputs(n, "normal", 80 + s)[0].to(DEV)
        out, out32 = torch.empty_like(g), torch.empty(n, dtype=torch.float32, device=DEV)
        ops.topk_residual_step(g, r, s > 0, 1.0, 1.0, k, out=out)
        ops.topk_residual_step(g.float(), r32, s > 0, 1.0, 1.0, k, out=out32)
        assert torch.equal(out.view(torch.int16), out32.to(BF16).view(torch.int16)), f"step {s}"
        assert torch.equal(r.view(torch.int32), r32.view(torch.int32)), f"residual, step {s}"


# ------------------------------------------------------------------------------- 7. refusals
def test_bf16_accepted_where_fp16_and_other_codecs_are_refused():
    """The entry points that take bf16 -- ops.topk_compress / topk_step_dense and grace_amd.torch's
    TopKCompressor.compress -- accept a bf16 tensor and raise TypeError on the same call with fp16.
    Every other codec (ThresholdCompressor here) still raises TypeError for bf16, and fp16 into
    grace_amd.dist's TopKCompressor raises as before (that class does not take bf16 either yet:
    DESIGN.md section 9, so its fp16 refusal alone tells nothing about bf16)."""
    from grace_amd import ops
    from grace_amd.dist.communicator.allgather import Allgather
    from grace_amd.dist.compressor.threshold import ThresholdCompressor
    from grace_amd.dist.compressor.topk import TopKCompressor
    from grace_amd.dist.memory.residual import ResidualMemory
    from grace_amd.torch.compressor.topk import TopKCompressor as HvdTopK
    x = torch.ones(4096, dtype=BF16, device=DEV)
    h = torch.ones(4096, dtype=torch.float16, device=DEV)
    # accepted as bf16, refused as fp16, by the same function
    assert ops.topk_compress(x, 40)[1].dtype == torch.float32
    with pytest.raises(TypeError):
        ops.topk_compress(h, 40)
    assert ops.topk_step_dense(x, 40)[3].dtype == BF16
    with pytest.raises(TypeError):
        ops.topk_step_dense(h, 40)
    assert HvdTopK(0.01).compress(x, "w")[0][0].numel() == 40
    with pytest.raises(TypeError):
        HvdTopK(0.01).compress(h, "w")
    with pytest.raises(TypeError):
        ThresholdCompressor(1.5).compress(x, "w")
    with pytest.raises(TypeError):
        TopKCompressor(0.01).compress(h, "w")
    with pytest.raises(TypeError):
        Allgather(TopKCompressor(0.01), ResidualMemory(), 1).step(h, "w")
    with pytest.raises(ValueError):      # no recycled output on bf16
        ops.topk_step_dense(x, 40, prev_idx=torch.zeros(40, dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError):      # a bf16 step's result is bf16
        ops.topk_step_dense(x, 40, out=torch.empty(4096, dtype=torch.float32, device=DEV))
    r = torch.empty(2 * 4096, dtype=torch.float32, device=DEV)
    with pytest.raises(ValueError):      # a strided residual would be written as if it were dense
        ops.topk_residual_step_swap(x, None, False, 1.0, 1.0, 40, r[::2])
    with pytest.raises(ValueError):
        ops.topk_residual_step(x, r[::2], False, 1.0, 1.0, 40)


def test_bf16_compress_horovod_flavour():
    """grace_amd.torch's TopKCompressor (int64 indices) compresses a bf16 tensor to the f32 payload."""
    from grace_amd.torch.compressor.topk import TopKCompressor
    n = 100003
    b, up = _inputs(n, "normal", n + 3)
    (vals, idx), ctx = TopKCompressor(0.01).compress(b.to(DEV), "w")
    assert idx.dtype == torch.int64 and ctx == (n, torch.Size([n]))
    check_topk(up, O.ratio_k(n, 0.01), vals, idx.to(torch.int32))
