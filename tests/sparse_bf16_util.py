"""Shared by the threshold / random-k bfloat16 tests (numpy / torch-CPU only): the constructed threshold
cases with the branch each one must land in, the reference steps on the widened gradient, the numpy
restatement of the padded decode, and the world-2 threshold gradients rounded to bf16."""
import numpy as np
import torch

from oracle import grace_oracle as O
from tests.dgc_bf16_util import bf16_pair
from tests.shard_select_util import round_cpu

F32 = np.float32
BETA, GAMMA, STEPS = 0.9, 0.7, 3     # t = beta r + gamma g is no bf16 number from step 2 on
THR = 1.5001      # just above a bf16 number: a selected t in [1.5001, 1.5039) rounds to 1.5, below it
THR_CASES = ["holds", "max_below", "neg_fixup", "all_negative", "nan", "thr0"]
THR_SIZES = [1, 7, 16384, 16389, 49154]   # one lane; scalar only; one whole chunk; a tail in a second
#                                           workgroup; three chunks and two elements


def bits16(out):
    """A bf16 tensor's 16-bit patterns as int32 numpy."""
    assert out.dtype == torch.bfloat16
    return (out.detach().contiguous().view(torch.int16).cpu().to(torch.int32) & 0xFFFF).numpy().ravel()


def want_bits(out32):
    """The f32 dense result rounded once (tests/shard_select_util.round_cpu) as int32 numpy."""
    return round_cpu(torch.from_numpy(np.ascontiguousarray(out32, dtype=F32))).numpy().ravel()


def bits32(x):
    return int(np.asarray(x, dtype=F32).reshape(1).view(np.uint32)[0])


def thr_of(case):
    return 0.0 if case == "thr0" else THR


def thr_feasible(case, n):
    return n >= 2 or case != "neg_fixup"     # a positive max beside a negative element needs two


def thr_grad(case, n, s):
    """Step s of the case's gradient sequence: Gaussian, shaped for the case's branch, with -0, bf16
    subnormals, +-inf and NaN planted, rounded to bf16 -> (CPU bf16 tensor, its f32 widening)."""
    rng = np.random.default_rng(1000 * len(case) + 10 * n + s)
    x = rng.standard_normal(n).astype(F32)
    odd = np.arange(n) % 2 == 1
    negative = case == "all_negative" or (case == "thr0" and s == 2)
    if case == "holds":
        x[0] = F32(2.5)                                     # max t >= thr whatever the rest is
    elif case == "max_below":
        x = np.abs(x) * F32(0.1) + F32(0.001)               # all positive: only the max reaches the bound
    elif case in ("neg_fixup", "nan"):
        x = np.where(odd, -np.abs(x) * F32(2.0), np.abs(x) * F32(0.1) + F32(0.001)).astype(F32)
        if n > 1:
            x[1] = F32(-3.0)                                # |t| >= thr at every step
    elif negative:
        x = -np.abs(x) - F32(0.25)
    if n >= 7:
        spots = [(2, -0.0), (4, 3e-39), (5, -9.2e-41)] + ([(n - 1, -0.0), (n - 3, -3e-39)] if n >= 16384 else [])
        for at, v in spots:
            if not negative or F32(v) < 0:                  # (-0 and a positive subnormal are not negative)
                x[at] = F32(v)
        if s == 2 and case in ("holds", "neg_fixup", "all_negative"):
            x[6] = -np.inf                                  # selected at thr: r' = NaN, which the fix-up leaves
            if case == "holds":
                x[3] = np.inf
    if case == "nan":
        x[n // 2] = np.nan
    return bf16_pair(x)


def thr_step(g, r, thr, residual=True, beta=BETA, gamma=GAMMA):
    """One Allgather(Threshold, ResidualMemory(beta, gamma) | NoneMemory, 1).step on the CPU ->
    dict(t, out f32, r', bound, count)."""
    with np.errstate(invalid="ignore", over="ignore"):
        t = O.residual_compensate(g, r, beta, gamma).ravel() if residual else np.asarray(g, dtype=F32).ravel()
        vals, idx = O.threshold_select(t, thr)
        dec = O.sparse_decode(vals, idx, t.size)
        out = (O.python_sum([dec]) / F32(1)).astype(F32)
        rn = O.residual_update(t, dec) if residual else None
        mx = F32(np.max(t)) if not np.isnan(t).any() else F32(np.nan)
        bound = mx if mx < F32(thr) else F32(thr)
    return dict(t=t, out=out, r=rn, bound=bound, count=int(idx.size), mx=mx)


def thr_check_branch(case, n, s, e, thr):
    """The constructed case really lands in its branch (the oracle's bound and count say so)."""
    t, mx, bound, count = e["t"], e["mx"], e["bound"], e["count"]
    thr = F32(thr)
    with np.errstate(invalid="ignore"):
        if case == "holds":
            assert mx >= thr and bits32(bound) == bits32(thr) and count >= 1
        elif case == "max_below":
            assert 0 < mx < thr and bits32(bound) == bits32(mx)
            assert count == int((t == mx).sum()) >= 1, "something else reached the bound"
        elif case == "neg_fixup":
            assert 0 < mx < thr and bits32(bound) == bits32(mx)
            assert (t <= -thr).any(), "no negative element of |t| >= thr"
            if n >= 16384:
                assert ((np.abs(t) >= mx) & (np.abs(t) < thr)).sum() > 1 and (np.abs(t) < mx).any()
            if s >= 1 and n >= 16384 and e["r"] is not None:
                # with memory, from the second step on: selected at thr with more than 8 significant bits
                sel = t[np.abs(t) >= thr]
                assert (sel.view(np.uint32) & 0xFFFF).any()
                # ... and some of them round to a bf16 below thr: a fix-up that asked the rounded output
                # whether the first pass had selected them would take them for elements left alone
                assert (np.abs(bf16_pair(sel)[1]) < thr).any(), "no selected element rounds below thr"
        elif case == "all_negative":
            assert mx < 0 and bits32(bound) == bits32(mx) and count == n
        elif case == "nan":
            assert np.isnan(t).any() and bits32(bound) == bits32(thr)
        elif case == "thr0":
            assert thr == 0
            if s == 2:
                assert mx < 0 and count == n
            else:
                assert n < 7 or (mx > 0 and bits32(bound) == bits32(thr))


# ------------------------------------------------------------------------------- the padded decode
def padded_ref(vals, idx, counts, cap, n, divisor):
    """numpy restatement of grace_sparse_aggregate_padded_bf16: vals f32[W][cap], idx i32[W][cap],
    counts[W] -> the f32 ((0 + d0) + d1 + ...) / divisor, to be rounded by want_bits.  Entries past
    min(max(count, 0), cap) do not exist; an index outside [0, n) is skipped."""
    acc = np.zeros(n, dtype=F32)
    for w in range(len(counts)):
        c = min(max(int(counts[w]), 0), cap)
        d = np.zeros(n, dtype=F32)
        i = np.asarray(idx[w][:c], dtype=np.int64)
        ok = (i >= 0) & (i < n)
        d[i[ok]] = np.asarray(vals[w][:c], dtype=F32)[ok]
        acc = (acc + d).astype(F32)
    with np.errstate(invalid="ignore", over="ignore"):
        return (acc / F32(divisor)).astype(F32) if divisor != 1 else acc


# ------------------------------------------------------------------------------- world 2
W2_N = 5003


def world2_thr_grad(kind, rank, s):
    """tests/test_gpu_world2.py's threshold gradients rounded to bf16 (as f32): `thr` (counts exchange,
    rank 1 twice as wide) and `cap` (capacity exchange, a 3x tail on rank 1 at step 2)."""
    if kind == "thr":
        g = np.random.default_rng(2000 * rank + s).standard_normal(W2_N).astype(F32) * (1 + rank)
    else:
        sc = 3.0 if s == 2 and rank == 1 else 1.0
        g = (np.random.default_rng(3000 * rank + s).standard_normal(W2_N) * sc).astype(F32)
    return bf16_pair(g)[1]
