"""Inputs of the DGC bfloat16 tests (numpy / torch-CPU only): gradients as bf16 tensors with their
exact f32 widening, tests/dgc_edge_util.py's threshold-loop cases with x rounded to bf16, and the
world-2 gradients of tests/test_gpu_dgc_world2.py rounded to bf16."""
import numpy as np
import torch

from tests.dgc_edge_util import LOOP_CASES, LoopCase

F32 = np.float32

# After rounding x to bf16, these still take the path their check() states ...
LOOP_PATH_HOLDS = ["ten_ups", "mixed_q90", "mixed_q97", "zigzag", "ties_at_thr0", "thr0_zero", "thr0_inf",
                   "large_finite", "tiny_1", "tiny_50", "tiny_99", "tiny_100", "tiny_101"]
# ... and these do not (a tie value that is no bf16 number, magnitudes that round to inf, bf16's
# 8 exponent bits with no subnormal f32 tail): they run against the oracle without the path assertion
LOOP_PATH_LOST = ["ties_at_a_later_node", "overflow_to_inf", "large_finite_unsettled", "subnormal"]


def bf16_pair(x):
    """f32 numpy array -> (the CPU bf16 tensor nearest to it, that tensor widened to f32 numpy)."""
    with np.errstate(over="ignore", invalid="ignore"):
        b = torch.from_numpy(np.ascontiguousarray(x, dtype=F32)).to(torch.bfloat16)
    return b, b.float().numpy()


def rounded_case(name):
    """LOOP_CASES[name] with x rounded to bf16 (as f32), the same sample indices and check."""
    c = LOOP_CASES[name]()
    return LoopCase(bf16_pair(c.x)[1], c.sidx, c._check, c.ratio)


W2_N = 50_000


def world2_grad(rank, step):
    """tests/test_gpu_dgc_world2.py's _grad, rounded to bf16 (as f32)."""
    rng = np.random.default_rng(4000 + 10 * rank + step)
    g = rng.standard_normal(W2_N, dtype=F32)
    if step == 3 and rank == 1:          # a heavier tail on one rank: more entries pass the threshold
        g[: W2_N // 3] *= F32(6.0)
    return bf16_pair(g)[1]
