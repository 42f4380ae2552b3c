"""ResidualMemory(beta, gamma) with factors other than 1 through every fused step that takes them
(grace_amd/csrc/topk.hip, sparse.hip): t = beta * r + gamma * g as two f32 multiplies and an add.
The unit case is its own template instantiation in the top-k main pass, so only non-unit factors
run the general one.  Every comparison is bit for bit against oracle/grace_oracle.py, whose
residual_compensate runs torch's CPU ops; every chain is three steps on one residual (the first
without a residual), so that a wrong r' shows in the next step's t."""
import numpy as np
import pytest
import torch

from oracle import grace_oracle as O
from tests.golden_util import same_bits
from tests.test_gpu_topk import _inputs, check_topk
from tests.topk_util import TopkChain, check_step, np_of as _np, to_dev as _t

pytestmark = pytest.mark.gpu
DEV = "cuda"
# both rounded; beta the unit alone; gamma the unit alone; 0 * inf and 0 * NaN must stay NaN
FACTORS = [(0.9, 0.5), (1.0, 0.1), (0.5, 1.0), (0.0, 1.0)]
MODES = ["out", "no_out", "swap"]


# ------------------------------------------------------------------------------- a. top-k, ops level
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kind", ["normal", "special"])
@pytest.mark.parametrize("beta,gamma", FACTORS)
@pytest.mark.parametrize("n", [1000, 32769, 100003])
def test_topk_step_factors(n, beta, gamma, kind, mode):
    """1000: the single-workgroup kernel (compensate in small_body); 32769: the smallest size on the
    three-kernel path (a whole chunk or two, then a partial one on the guarded loads); 100003: several
    whole fast chunks at both chunk lengths (12288 and 20480), a partial chunk and a 3-element tail.
    The swap step's finalize recomputes t from g and r_in (MainTs), so a main pass with a wrong t
    there only makes the candidate counts disagree and the exact fallback repairs the result: on
    the three-kernel path the steps on normal inputs must also stay on the sampled path."""
    from grace_amd import ops
    k = O.ratio_k(n, 0.01)
    chain = TopkChain(mode, n)
    res = None
    for s in range(3):
        g0 = _inputs(n, kind, 300 + 10 * s + n % 7)
        vals, idx = chain.step(g0, s > 0, beta, gamma, k)
        t, _, _, res, oout = O.topk_residual_step(g0, res, None, beta=beta, gamma=gamma, k=k)
        check_step(chain, t, k, vals, idx, res, oout, s)
        if n > 32768 and kind == "normal":
            assert ops.topk_status(n, k, torch.device(DEV, 0)) == 0, (s, "took the exact fallback")


def test_topk_step_factors_unaligned_views():
    """g, r and out one element into larger buffers: no 16-byte alignment, so every chunk takes the
    guarded (non-vector) path with factors; the element before each view stays as it was."""
    from grace_amd import ops
    n, beta, gamma = 100003, 0.9, 0.5
    k = O.ratio_k(n, 0.01)
    gbuf, rbuf, obuf = (torch.full((n + 1,), 7.0, device=DEV) for _ in range(3))
    res = None
    for s in range(3):
        g0 = _inputs(n, "special", 330 + s)
        gbuf[1:].copy_(_t(g0))
        _, vals, idx = ops.topk_residual_step(gbuf[1:], rbuf[1:], s > 0, beta, gamma, k, out=obuf[1:])
        t, _, _, res, oout = O.topk_residual_step(g0, res, None, beta=beta, gamma=gamma, k=k)
        check_topk(t, k, vals, idx)
        assert same_bits(_np(rbuf[1:]), res), s
        assert same_bits(_np(obuf[1:]), oout), s
        assert [float(b[0]) for b in (gbuf, rbuf, obuf)] == [7.0, 7.0, 7.0], s


# ------------------------------------------------------------------------------- b. exact fallback
def _sparse_pair(n, rng, neg_zero):
    """(g, r): n // 800 non-zeros each, at different positions; with neg_zero, -0.0 in BOTH at some
    low zero positions (beta r + gamma g is -0 only where both terms are)."""
    pos = rng.choice(n, size=2 * (n // 800), replace=False)
    g, r = np.zeros(n, np.float32), np.zeros(n, np.float32)
    g[pos[:n // 800]] = rng.standard_normal(n // 800).astype(np.float32)
    r[pos[n // 800:]] = rng.standard_normal(n // 800).astype(np.float32)
    if neg_zero:
        low = np.setdiff1d(np.arange(200), pos)[::3]
        g[low] = -0.0
        r[low] = -0.0
    return g, r


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("beta,gamma", [(0.9, 0.5), (0.5, 1.0)])
@pytest.mark.parametrize("n", [70001, 100003])
def test_topk_exact_fallback_factors(n, beta, gamma, mode):
    """k above the non-zeros of t: the bracket cannot hold and the exact fallback selects from t as
    it recomputes it (MainTs: from g and the untouched r_in in the swap step, with the factors), which
    must be the main pass's t bit for bit.  The residual is explicit and sparse from the first call.
    A fallback step selects every non-zero, so its residual is all zeros: the second step gets fresh
    non-zeros planted in the residual (on both sides) besides a fresh sparse g."""
    from grace_amd import ops
    k = n // 100
    rng = np.random.default_rng(n + int(10 * beta))
    neg_zero = mode == "out"
    g0, r0 = _sparse_pair(n, rng, neg_zero)
    chain = TopkChain(mode, n, r0=r0)
    res = r0
    for s in range(2):
        if s == 1:
            g0, plant = _sparse_pair(n, rng, neg_zero)
            assert not np.any(res), "a fallback step leaves no non-zero residual"
            res = plant
            chain.residual.copy_(_t(plant))
        t, ov, _, ores, oout = O.topk_residual_step(g0, res, None, beta=beta, gamma=gamma, k=k)
        assert 0 < np.count_nonzero(t) < k and np.count_nonzero(res) and np.count_nonzero(g0)
        if neg_zero:
            assert np.any(np.signbit(ov) & (ov == 0)), "-0 is among the selected ties"
        vals, idx = chain.step(g0, True, beta, gamma, k)
        torch.cuda.synchronize()
        assert ops.topk_status(n, k, torch.device(DEV, 0)) == 1, s
        check_step(chain, t, k, vals, idx, ores, oout, s)
        res = ores


# ------------------------------------------------------------------------------- c. carry live
CARRY_N = 1 << 24


def _carry_g(s):
    return _inputs(CARRY_N, "special", 500 + s)


@pytest.fixture(scope="module")
def carry_oracle():
    """The three oracle steps at 2^24 elements (about 0.5 s each), computed once for both modes.
    Kept until the module is done: t, the residual and the result of each step, 64 MiB apiece
    (576 MiB of host memory); the gradients are drawn again from their seeds instead."""
    k = O.ratio_k(CARRY_N, 0.01)
    res, steps = None, []
    for s in range(3):
        t, _, _, res, oout = O.topk_residual_step(_carry_g(s), res, None, beta=0.9, gamma=0.5, k=k)
        for a in (t, res, oout):       # shared by both modes: read-only
            a.setflags(write=False)
        steps.append((t, res, oout))
    return steps


@pytest.mark.parametrize("mode", ["out", "swap"])
def test_topk_carry_live_factors(mode, carry_oracle):
    """2^24 elements, the smallest bucket whose bracket keeps a residual-sample carry: from the
    second step the bracket rebuilds r'(pos) from the carried t and threshold and computes
    t = beta r' + gamma g itself.  That line only places the bracket (a misplaced one takes the exact
    fallback and still gives the exact result), so the steps must also stay on the sampled path."""
    from grace_amd import ops
    n, k = CARRY_N, O.ratio_k(CARRY_N, 0.01)
    size = ops.topk_carry_size(n, k)
    assert size > 0
    chain = TopkChain(mode, n, carry=torch.full((size,), float("nan"), device=DEV))
    for s, (t, ores, oout) in enumerate(carry_oracle):
        vals, idx = chain.step(_carry_g(s), s > 0, 0.9, 0.5, k)
        torch.cuda.synchronize()
        status = ops.topk_status(n, k, torch.device(DEV, 0))
        check_step(chain, t, k, vals, idx, ores, oout, s)
        assert status == 0, (s, status, "a valid carry keeps the sampled path")


# ------------------------------------------------------------------------------- d. recycled output
def test_topk_recycled_output_factors():
    """recycle_output="always": the SPARSE main pass (the dropped previous result comes back, only
    the selection is written) beside the dense-write step, both against the oracle."""
    from grace_amd.dist.communicator.allgather import Allgather
    from grace_amd.dist.compressor.topk import TopKCompressor
    from grace_amd.dist.memory.residual import ResidualMemory
    n, beta, gamma = 100003, 0.9, 0.5
    rec = Allgather(TopKCompressor(0.01, recycle_output="always"), ResidualMemory(beta, gamma), 1)
    ref = Allgather(TopKCompressor(0.01, recycle_output=False), ResidualMemory(beta, gamma), 1)
    res, recycled = None, 0
    for s in range(4):
        g0 = _inputs(n, "special" if s % 2 else "normal", 600 + s)
        before = rec.compressor._recycler._hit.get("b")
        o1 = rec.step(_t(g0), "b")
        if before is not None and o1.data_ptr() == before[0].data_ptr():
            recycled += 1
        o2 = ref.step(_t(g0), "b")
        _, _, _, res, oout = O.topk_residual_step(g0, res, 0.01, beta=beta, gamma=gamma)
        assert same_bits(_np(o1), oout), s
        assert same_bits(_np(o2), oout), s
        assert same_bits(_np(rec.memory.residuals["b"]), res), s
        assert same_bits(_np(ref.memory.residuals["b"]), res), s
        del o1, o2                            # dropped: the next step may recycle it
    assert recycled >= 1


# ------------------------------------------------------------------------------- e. dist layer
@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("beta,gamma", FACTORS)
def test_allgather_topk_residual_factors(beta, gamma, fused):
    """Allgather(TopK, ResidualMemory(beta, gamma), 1): the fused step, and the reference's four
    calls (compensate, compress, update, send_receive)."""
    from grace_amd.dist.communicator.allgather import Allgather
    from grace_amd.dist.compressor.topk import TopKCompressor
    from grace_amd.dist.memory.residual import ResidualMemory
    n = 100003
    comm = Allgather(TopKCompressor(0.01), ResidualMemory(beta, gamma), 1)
    res = None
    for s in range(3):
        g0 = _inputs(n, "special" if s == 1 else "normal", 700 + s)
        g = _t(g0)
        if fused:
            out = comm.step(g, "b")
        else:
            t = comm.memory.compensate(g, "b")
            payload, ctx = comm.compressor.compress(t, "b")
            comm.memory.update(t, "b", comm.compressor, payload, ctx)
            out = comm.send_receive(payload, "b", ctx)
        _, _, _, res, oout = O.topk_residual_step(g0, res, 0.01, beta=beta, gamma=gamma)
        assert same_bits(_np(out).ravel(), oout), s
        assert same_bits(_np(comm.memory.residuals["b"]).ravel(), res), s


# ------------------------------------------------------------------------------- f. segmented
SEG_SIZES = [3, 40000, 5, 50001, 8193, 20000, 8192, 1, 1 << 20]
CTL_WORDS, CTL_STATUS = 16, 3       # topk.hip TopkCtl: 16 32-bit words, `status` the fourth


@pytest.mark.parametrize("dense", [True, False])
@pytest.mark.parametrize("beta,gamma", [(0.9, 0.5), (0.5, 1.0)])
def test_segmented_factors(beta, gamma, dense):
    """SegmentedTopK with factors: small segments (one workgroup each), large ones at odd offsets
    (the prep kernel's bracket, main pass and finalize per segment) and one of 2^20 elements, whose
    bracket keeps the per-segment carry; special values in one large segment.  `step` writes the
    dense result, `local_step` the residual only; checked per tensor.
    From the second step the prep kernel rebuilds r'(pos) of the 2^20 segment from its carry and
    computes t = beta r' + gamma g itself, which only places that segment's bracket (a misplaced one
    takes the segment's exact fallback, with the same result).  So that the place depends on beta,
    that segment's gradient is small next to its residual after the first step, and the segment
    must stay on the sampled path (status word of its workspace: topk.hip TopkCtl)."""
    from grace_amd.dist.segmented import SegmentedTopK
    ratio = 0.01
    eng = SegmentedTopK(ratio)
    eng.beta, eng.gamma = beta, gamma                 # the engine's ResidualMemory factors
    rng = np.random.default_rng(int(100 * beta) + dense)
    res = [None] * len(SEG_SIZES)
    for s in range(3):
        gs = [rng.standard_normal(n).astype(np.float32) for n in SEG_SIZES]
        gs[3][[0, 7, 77, 777, 50000]] = [np.nan, np.inf, -np.inf, -0.0, np.nan]
        if s > 0:
            gs[-1] *= np.float32(0.01)
        flat = _t(np.concatenate(gs))
        if dense:
            out = _np(eng.step(flat, SEG_SIZES))
        else:
            eng.local_step(flat, SEG_SIZES)
        ntab = len(eng._tables)
        T = eng.tables(SEG_SIZES, flat.device, s > 0, dense)
        assert len(eng._tables) == ntab, "not the tables (and workspace) the step itself used"
        li = T["large"].cpu().tolist()[:T["n_large"]].index(len(SEG_SIZES) - 1)
        ctl = int(T["ws_off"].cpu()[li])                           # the segment's TopkCtl block
        status = int(T["ws"][ctl:ctl + 4 * CTL_WORDS].view(torch.int32).cpu()[CTL_STATUS])
        assert status == 0, (s, status, "a valid carry keeps the segment on the sampled path")
        vals, idx = (_np(x) for x in eng.last_payload)
        idx = idx.astype(np.int64)
        rcat = _np(eng.residuals["bucket"])
        off = koff = 0
        for j, g in enumerate(gs):
            n = g.size
            _, v_or, i_or, res[j], o = O.topk_residual_step(g, res[j], ratio, beta=beta, gamma=gamma)
            if dense:
                assert same_bits(out[off:off + n], o), (s, j)
            k = i_or.size
            mine = idx[koff:koff + k] - off
            order = np.argsort(mine)
            assert np.array_equal(mine[order], i_or.astype(np.int64)), (s, j)
            assert same_bits(vals[koff:koff + k][order], v_or), (s, j)
            assert same_bits(rcat[off:off + n], res[j]), (s, j)
            off += n
            koff += k


# ------------------------------------------------------------------------------- g. random-k
def _planted(n, rng):
    g = rng.standard_normal(n).astype(np.float32)
    g[rng.choice(n, 3, replace=False)] = np.nan
    g[rng.choice(n, 3, replace=False)] = -np.inf
    g[rng.choice(n, 20, replace=False)] = -0.0
    return g


@pytest.mark.parametrize("beta,gamma", FACTORS)
@pytest.mark.parametrize("ratio", [0.05, 0.7])
@pytest.mark.parametrize("n", [4097, 100003])
def test_randomk_steps_factors(n, ratio, beta, gamma):
    """ops.randomk_step_w1, ops.randomk_step_w1_dense and ops.randomk_shard_step (two shards of one
    bucket, the second at an odd offset) against the oracle sequence compensate -> t[idx] -> decode
    -> update, out = 0 + decode; indices drawn with replacement (ratio 0.7: many duplicates).  Two
    steps on one residual each: without a residual (the buffer holds NaN and must not be read), then
    with the first step's."""
    from grace_amd import ops
    rng = np.random.default_rng(n + int(100 * ratio) + int(10 * beta))
    k = O.ratio_k(n, ratio)
    m0 = n // 2 + 1                                           # shards [0, m0) and [m0, n)
    r_w1, r_dense, r_shard = (torch.full((n,), float("nan"), device=DEV) for _ in range(3))
    res = None
    for has in (False, True):
        g0 = _planted(n, rng)
        idx0 = rng.integers(0, n, k).astype(np.int64)
        t = O.residual_compensate(g0, res, beta, gamma)
        ovals = t[idx0]
        dec = O.randomk_decode(ovals, idx0, n)
        res = O.residual_update(t, dec)
        oout = O.python_sum([dec])
        g, idx = _t(g0), _t(idx0)
        vals, out = ops.randomk_step_w1(g, r_w1, has, beta, gamma, idx)
        assert same_bits(_np(vals), ovals), has
        assert same_bits(_np(out), oout), has
        assert same_bits(_np(r_w1), res), has
        out = ops.randomk_step_w1_dense(g, r_dense, has, beta, gamma, idx)
        assert same_bits(_np(out), oout), ("dense", has)
        assert same_bits(_np(r_dense), res), ("dense", has)
        out = torch.full((n,), float("nan"), device=DEV)
        for lo, hi in ((0, m0), (m0, n)):
            vals = ops.randomk_shard_step(g[lo:hi], r_shard[lo:hi], has, beta, gamma, lo, idx, out=out[lo:hi])
            mine = (idx0 >= lo) & (idx0 < hi)
            assert same_bits(_np(vals), np.where(mine, ovals, np.float32(0.0)).astype(np.float32)), ("shard", lo, has)
        assert same_bits(_np(out), oout), ("shard", has)
        assert same_bits(_np(r_shard), res), ("shard", has)


# ------------------------------------------------------------------------------- h. threshold
@pytest.mark.parametrize("nan", [False, True])
@pytest.mark.parametrize("beta,gamma", FACTORS)
@pytest.mark.parametrize("n", [5000, 16384 * 3 + 5])
def test_threshold_step_factors(n, beta, gamma, nan):
    """Allgather(Threshold 1.5, ResidualMemory(beta, gamma), 1).step (grace_threshold_step_w1): whole
    16384-element chunks plus a ragged one with a scalar tail.  The second step is all-negative, so
    max t < thr and the fix-up pass rebuilds t from what the speculative pass wrote; with NaN planted
    the bound stays at thr."""
    from grace_amd.dist.communicator.allgather import Allgather
    from grace_amd.dist.compressor.threshold import ThresholdCompressor
    from grace_amd.dist.memory.residual import ResidualMemory
    thr = 1.5
    comm = Allgather(ThresholdCompressor(thr), ResidualMemory(beta, gamma), 1)
    rng = np.random.default_rng(n + int(10 * beta) + nan)
    res = None
    for s in range(3):
        x = rng.standard_normal(n).astype(np.float32)
        x[-8:] = np.float32(0.125) * (1 + np.arange(8, dtype=np.float32))   # below thr: the tail's residual stays live
        if s == 1:
            x = -np.abs(x)
        if nan:
            x[rng.choice(n - 8, 3, replace=False)] = np.nan
        out = _np(comm.step(_t(x), "w"))
        t = O.residual_compensate(x, res, beta, gamma)
        if s == 1 and not nan:
            assert np.max(t) < thr                            # the fix-up pass runs
        ov, oi = O.threshold_select(t, thr)
        dec = O.sparse_decode(ov, oi, n)
        assert same_bits(out, (O.python_sum([dec]) / np.float32(1)).astype(np.float32)), s
        res = O.residual_update(t, dec)
        assert same_bits(_np(comm.memory.residuals["w"]), res), s
