"""Inputs that drive DgcCompressor.compress's threshold adjustment loop (dgc.py:28-36) down chosen
paths, with the property each must have stated as a check on the oracle's trace -- shared by
tests/test_gpu_dgc_edges.py (the engine against the oracle on them) and tests/test_dgc_edge_cases.py
(the constructions themselves, on the CPU).  Every sample index lies in [0, n)."""
import numpy as np

from oracle import grace_oracle as O

F32 = np.float32
N, RATIO = 40000, 0.01          # ns = 400, ks = 4, bounds 280 and 520
FLT_MIN = F32(1.17549435e-38)    # the smallest normal f32


def ns_of(n):
    return max(1, int(n * 0.01))


def bits(v):
    return int(np.asarray(v, dtype=F32).reshape(1).view(np.uint32)[0])


class LoopCase:
    """x (f32), sidx (int64, ns entries), ratio, and check(trace): the path property."""

    def __init__(self, x, sidx, check, ratio=RATIO):
        self.x = np.ascontiguousarray(x, dtype=F32)
        self.sidx = np.ascontiguousarray(sidx, dtype=np.int64)
        self.ratio = ratio
        self._check = check
        n = self.x.size
        assert self.sidx.size == ns_of(n) and self.sidx.min() >= 0 and self.sidx.max() < n

    def bounds(self):
        n = self.x.size
        return F32(0.7 * n * self.ratio), F32(1.3 * n * self.ratio)

    def check_path(self):
        """Assert that the oracle's loop takes the path this input was built for; returns the trace."""
        trace = O.dgc_adjust_trace(self.x, self.sidx, self.ratio)
        path = "".join(m for m, _, _ in trace)
        assert path == O.dgc_adjust_path(self.x, self.sidx, self.ratio)
        self._check(self, path, trace)
        return trace


def _gauss(n=N, seed=1):
    return np.random.default_rng(seed).standard_normal(n).astype(F32)


def _settled(case, trace):
    lo, hi = case.bounds()
    return lo <= F32(trace[-1][2]) <= hi


def alternations(path):
    return sum(a != b for a, b in zip(path, path[1:]))


def ten_ups():
    x = _gauss()
    sidx = np.argsort(np.abs(x), kind="stable")[:ns_of(N)]

    def check(c, path, trace):
        assert path == "U" * 10 and not _settled(c, trace)
        assert trace[-1][2] > 30000          # about 34,700 of 40,000 stay selected

    return LoopCase(x, sidx, check)


def mixed(q):
    x = _gauss()
    at = np.argsort(np.abs(x), kind="stable")[int(q * N)]
    sidx = np.full(ns_of(N), at)

    def check(c, path, trace):
        assert len(path) >= 3 and "U" in path and "D" in path and _settled(c, trace), path

    return LoopCase(x, sidx, check)


def zigzag():
    rng = np.random.default_rng(1)
    x = (rng.standard_normal(N) * 1e-3).astype(F32)
    ones = rng.choice(N, 2000, replace=False)
    x[ones] = np.where(rng.random(2000) < 0.5, F32(-1.0), F32(1.0))
    sidx = rng.choice(ones, ns_of(N))

    def check(c, path, trace):
        assert bits(trace[0][1]) == bits(1.0) and trace[0][2] == 2000       # ties exactly on a table value
        assert len(path) == 10 and alternations(path) >= 4, path
        assert trace[-1][2] == 0                                            # an empty payload

    return LoopCase(x, sidx, check)


def ties(later_node):
    """Ties that decide the result (the zigzag's only reorder its path).  400 entries of exactly
    +-v over small noise, where v is the threshold the loop settles on: v = thr0 = 1.0 sampled
    from those entries themselves, or (later_node) v = f32(1.3) * 1.0, reached by one move up from
    2,000 sampled entries of +-1.0.  The count at v is in the band only if every tie is counted."""
    rng = np.random.default_rng(2)
    x = (rng.standard_normal(N) * 1e-3).astype(F32)
    pick = rng.choice(N, 2400, replace=False)
    sign = np.where(rng.random(2400) < 0.5, F32(-1.0), F32(1.0))
    v = F32(F32(1.3) * F32(1.0)) if later_node else F32(1.0)
    x[pick[:400]] = sign[:400] * v
    if later_node:
        x[pick[400:]] = sign[400:]
    sidx = rng.choice(pick[400:] if later_node else pick[:400], ns_of(N))

    def check(c, path, trace):
        assert path == ("U" if later_node else ""), path
        assert bits(trace[0][1]) == bits(1.0) and bits(trace[-1][1]) == bits(v) and trace[-1][2] == 400
        assert int((np.abs(c.x) > v).sum()) == 0           # nothing but the ties is selected

    return LoopCase(x, sidx, check)


def thr0_zero():
    rng = np.random.default_rng(1)
    x = np.zeros(N, dtype=F32)
    pick = rng.choice(N, 2000 + 300 + 1, replace=False)
    x[pick[:2000]] = 3.0
    x[pick[2000:2300]] = -0.0
    x[pick[2300]] = np.nan
    zeros = np.flatnonzero(x == 0)                     # +0 and -0
    sidx = rng.choice(zeros, ns_of(N))
    assert np.signbit(x[sidx]).any() and not np.signbit(x[sidx]).all()

    def check(c, path, trace):
        assert path == "U" * 10
        assert all(bits(thr) == 0 for _, thr, _ in trace)                   # thr stays +0
        assert trace[-1][2] == N - 1                                        # all but the NaN, +-0 included

    return LoopCase(x, sidx, check)


def thr0_inf():
    rng = np.random.default_rng(1)
    x = _gauss()
    infs = rng.choice(N, 7, replace=False)
    x[infs] = [np.inf, -np.inf, np.inf, -np.inf, -np.inf, np.inf, -np.inf]
    sidx = np.full(ns_of(N), infs[1])

    def check(c, path, trace):
        assert path == "D" * 10
        assert all(bits(thr) == bits(np.inf) and cnt == 7 for _, thr, cnt in trace)

    return LoopCase(x, sidx, check)


def overflow_to_inf():
    rng = np.random.default_rng(1)
    x = (rng.uniform(2e38, 3.4e38, N) * np.where(rng.random(N) < 0.5, -1.0, 1.0)).astype(F32)
    assert np.isfinite(x).all()
    at = np.argsort(np.abs(x), kind="stable")[N // 2]
    sidx = np.full(ns_of(N), at)

    def check(c, path, trace):
        assert len(path) == 10 and path[0] == "U"
        first_inf = next(i for i, (_, thr, _) in enumerate(trace) if np.isinf(thr))
        assert 1 <= first_inf <= 2 and path[first_inf:] == "D" * (10 - first_inf), path
        assert bits(trace[-1][1]) == bits(np.inf) and trace[-1][2] == 0

    return LoopCase(x, sidx, check)


def large_finite(seed):
    """seed 2: the median magnitude times 1.3^5 lands in the band (settles); seed 1: it misses
    the band on both sides, so the loop goes on alternating just below FLT_MAX for all 10 moves"""
    with np.errstate(over="ignore"):
        x = (np.random.default_rng(seed).standard_normal(N) * 1e38).astype(F32)   # a few overflow to +-inf
    at = np.argsort(np.abs(x), kind="stable")[N // 2]
    sidx = np.full(ns_of(N), at)

    def check(c, path, trace):
        assert len(path) >= 3 and path[:3] == "UUU", path
        assert np.isfinite(trace[-1][1]) and trace[-1][1] > F32(1e38)
        if seed == 2:
            assert len(path) < 10 and _settled(c, trace), path
        else:
            assert len(path) == 10 and alternations(path) >= 3, path

    return LoopCase(x, sidx, check)


def subnormal():
    rng = np.random.default_rng(1)
    x = (rng.standard_normal(N) * 1e-42).astype(F32)
    sidx = rng.integers(0, N, ns_of(N))

    def check(c, path, trace):
        assert 0 < trace[0][1] < FLT_MIN and 0 < trace[-1][1] < FLT_MIN      # thr0 and thr subnormal

    return LoopCase(x, sidx, check)


def tiny(n):
    rng = np.random.default_rng(n)
    x = rng.standard_normal(n).astype(F32)
    sidx = rng.integers(0, n, 1)
    assert ns_of(n) == 1

    def check(c, path, trace):
        if n in (1, 50):      # 1.3 n ratio < 1: a count of 1 is too many, 0 too few -- never settles
            assert c.bounds()[1] < 1 and len(path) == 10, path

    return LoopCase(x, sidx, check)


LOOP_CASES = {
    "ten_ups": ten_ups,
    "mixed_q90": lambda: mixed(0.90),
    "mixed_q97": lambda: mixed(0.97),
    "zigzag": zigzag,
    "ties_at_thr0": lambda: ties(False),
    "ties_at_a_later_node": lambda: ties(True),
    "thr0_zero": thr0_zero,
    "thr0_inf": thr0_inf,
    "overflow_to_inf": overflow_to_inf,
    "large_finite": lambda: large_finite(2),
    "large_finite_unsettled": lambda: large_finite(1),
    "subnormal": subnormal,
    "tiny_1": lambda: tiny(1),
    "tiny_50": lambda: tiny(50),
    "tiny_99": lambda: tiny(99),
    "tiny_100": lambda: tiny(100),
    "tiny_101": lambda: tiny(101),
}
