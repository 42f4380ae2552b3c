"""The HIP top-k engine (grace_amd/csrc/topk.hip) at the ends of k, in f32, bit for bit against the
oracle.  The sampled bracket has other regimes there than at the ratios the rest of the suite
uses: at k = 1 or 2 nothing is "sure" (the band is open at the top); from k = n / 2 the candidate
capacity min(2k + 65536, n) saturates at n and most elements are flagged in the main pass (the
wave-region spill); at k = n - 1 the band is open at the bottom; k = n on a bucket past the
single-workgroup size selects everything in index order (topk_all), and in the single-workgroup
kernel skips the select."""
import numpy as np
import pytest
import torch

from oracle import grace_oracle as O
from tests import test_gpu_topk_bf16 as B
from tests.golden_util import same_bits
from tests.test_gpu_topk import _inputs, check_topk
from tests.topk_util import TopkChain, check_step, np_of as _np, to_dev as _t

pytestmark = pytest.mark.gpu
DEV = "cuda"
SMALL_N = 32768          # topk.hip kSmallN: up to here one workgroup does everything
SIZES = [1, 2, 5, 1000, 32768, 32769, 100003]


def _ks(n):
    return sorted({min(n, max(1, k)) for k in (1, 2, n // 2, n - 1, n)})


CASES = [(n, k) for n in SIZES for k in _ks(n)]


def _edge_inputs(n, kind, seed):
    """tests/test_gpu_topk.py::_inputs; its 'special' plants 65 values, so below that size the
    specials are laid out by hand."""
    if kind == "special" and n < 1000:
        return np.resize(np.array([np.nan, -0.0, np.inf, -1.5, -np.inf, 0.25], dtype=np.float32), n)
    return _inputs(n, kind, seed)


@pytest.mark.parametrize("kind", ["normal", "ties", "special"])
@pytest.mark.parametrize("n,k", CASES)
def test_topk_k_edges(n, k, kind):
    """ops.topk_compress, ops.topk_step_dense and ops.topk_residual_step (with a residual and a
    dense output): payload, residual and output."""
    from grace_amd import ops
    x = _edge_inputs(n, kind, 900 + n % 11 + k % 5)
    ordered = k == n and n > SMALL_N       # topk_all writes the payload in index order
    xt = _t(x)
    _, vals, idx = ops.topk_compress(xt, k)
    check_topk(x, k, vals, idx)
    if ordered:
        assert np.array_equal(_np(idx), np.arange(n))
    _, vals, idx, out = ops.topk_step_dense(xt, k)
    check_topk(x, k, vals, idx)
    assert same_bits(_np(out), np.float32(0.0) + O.sparse_decode(*O.topk_select(x, k), n))
    assert same_bits(_np(xt), x), "the input was modified"
    r0 = (np.float32(0.1) * _edge_inputs(n, "normal", 901 + n % 11)).astype(np.float32)
    r, out = _t(r0), torch.empty(n, device=DEV)
    _, vals, idx = ops.topk_residual_step(xt, r, True, 1.0, 1.0, k, out=out)
    t, _, _, ores, oout = O.topk_residual_step(x, r0, None, k=k)
    check_topk(t, k, vals, idx)
    if ordered:
        assert np.array_equal(_np(idx), np.arange(n))
    assert same_bits(_np(r), ores)
    assert same_bits(_np(out), oout)


def test_topk_half_the_bucket_swap():
    """k = n / 2 through ops.topk_residual_step_swap (provisional picks zeroed in the main pass, most
    of the bucket flagged), first without a residual, then with."""
    n = 100003
    k = n // 2
    chain = TopkChain("swap", n)
    res = None
    for s in range(2):
        g0 = _inputs(n, "ties" if s else "normal", 950 + s)
        vals, idx = chain.step(g0, s > 0, 1.0, 1.0, k)
        t, _, _, res, oout = O.topk_residual_step(g0, res, None, k=k)
        check_step(chain, t, k, vals, idx, res, oout, s)


@pytest.mark.parametrize("k", [1, 32768])
def test_bf16_k_edges(k):
    """The bf16 counterparts at n = 32769 (k = 1 and k = n - 1): compress, the no-memory step and
    the residual step with a bf16 result."""
    from grace_amd import ops
    n = 32769
    b, up = B._inputs(n, "special", 960 + k % 7)
    xd = b.to(DEV)
    _, vals, idx = ops.topk_compress(xd, k)
    B.check_topk(up, k, vals, idx)
    _, vals, idx, out = ops.topk_step_dense(xd, k)
    B.check_topk(up, k, vals, idx)
    B.check_dense(out, np.float32(0.0) + O.sparse_decode(*O.topk_select(up, k), n))
    r0 = (np.float32(0.1) * _inputs(n, "normal", 961)).astype(np.float32)
    r, out = _t(r0), torch.empty(n, dtype=torch.bfloat16, device=DEV)
    _, vals, idx = ops.topk_residual_step(xd, r, True, 1.0, 1.0, k, out=out)
    t, ores, exp_out, _ = B._oracle_step(up, r0, k)
    B.check_topk(t, k, vals, idx)
    assert same_bits(_np(r), ores)
    B.check_dense(out, exp_out)
