"""Helpers shared by the top-k GPU tests that step one residual through several calls."""
import numpy as np
import torch

from tests.golden_util import same_bits

DEV = "cuda"


def np_of(t):
    return t.detach().cpu().numpy()


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


class TopkChain:
    """One residual stepped through ops.topk_residual_step (with or without a dense output) or
    through ops.topk_residual_step_swap (two buffers in turn; r_in must come back unchanged)."""

    def __init__(self, mode, n, r0=None, carry=None):
        self.mode, self.n, self.carry, self.steps = mode, n, carry, 0
        first = torch.zeros(n, device=DEV) if r0 is None else to_dev(r0)
        self.bufs = [first, torch.zeros(n, device=DEV)] if mode == "swap" else [first]
        self.out = torch.empty(n, device=DEV) if mode == "out" else None

    @property
    def residual(self):
        return self.bufs[self.steps % len(self.bufs)]

    def step(self, g0, has, beta, gamma, k):
        from grace_amd import ops
        g = to_dev(g0)
        kw = {} if self.carry is None else {"carry": self.carry, "carry_valid": self.steps > 0}
        if self.mode == "swap":
            r_in, r_out = self.bufs[self.steps % 2], self.bufs[(self.steps + 1) % 2]
            before = np_of(r_in).copy()
            _, vals, idx = ops.topk_residual_step_swap(g, r_in, has, beta, gamma, k, r_out, **kw)
            torch.cuda.synchronize()
            assert same_bits(np_of(r_in), before), "r_in was written"
        else:
            _, vals, idx = ops.topk_residual_step(g, self.bufs[0], has, beta, gamma, k, out=self.out, **kw)
        self.steps += 1
        return vals, idx


def check_step(chain, t, k, vals, idx, ores, oout, where):
    """Payload against the oracle's selection from t; the chain's residual and dense output."""
    from tests.test_gpu_topk import check_topk
    check_topk(t, k, vals, idx)
    assert same_bits(np_of(chain.residual), ores), (where, "residual differs")
    if chain.out is not None:
        assert same_bits(np_of(chain.out), oout), (where, "dense output differs")
