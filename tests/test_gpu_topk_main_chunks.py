"""The top-k main pass with several chunks per workgroup (grace_topk_main_grid_limit; DESIGN §4 "One
reservation per chunk"): a workgroup that takes more than one chunk flushes its staged lists after
every chunk -- both lists reserved by one 64-bit add -- and keeps one LDS histogram for all of them.
Whatever the grid, every dense output, residual and payload must equal the oracle's
Allgather(TopK, ResidualMemory).step (grace_dl/dist/compressor/topk.py:32-69, memory/residual.py:10-20)
bit for bit, and the result under a capped grid must equal the default grid's.

A chunk is 12,288 elements, the large path starts above 32,768: the sizes are the smallest at which
each path exists.  Grid limits 1, 2, 3: one workgroup takes every chunk; even and odd splits; a
workgroup whose last chunk has no successor.  0 is the shipped default."""
import functools

import numpy as np
import pytest
import torch

from oracle import grace_oracle as O
from tests.golden_util import same_bits
from tests.test_gpu_out_lines import _Steps, _gradient, _map_of, _np, _t

pytestmark = pytest.mark.gpu
DEV = "cuda"
CHUNK = 12288
ROW = 1024                 # elements of one row of a chunk (256 lanes x 4)
WAVE_ROW = 256             # ... of which a wave holds 256
LIST_WAVE = 512            # a wave's staged-list region (kListWave)
LIMITS = [1, 2, 3, 0]
# three whole chunks; three FAST chunks and a tail chunk in the same workgroup; five chunks; five and
# a tail; all tail
SIZES = [36864, 36869, 61440, 61443, 32772]
NORMAL4 = ("normal",) * 4


@pytest.fixture(autouse=True)
def _default_grid():
    from grace_amd import ops
    yield
    ops.topk_main_grid_limit(0)


def _wave_share(chunk, wave):
    """The elements of chunk `chunk` that wave `wave` of its workgroup classifies."""
    rows = np.arange(CHUNK // ROW)[:, None] * ROW
    return (chunk * CHUNK + rows + wave * WAVE_ROW + np.arange(WAVE_ROW)[None, :]).ravel()


def _band_gradient(n, seed, res, ratio, beta, gamma, chunk, wave):
    """Like the "const" gradient, on a 5 % subset only: one constant magnitude just under the k-th
    magnitude of the rest, on every element of one wave's share of one chunk -- thousands of equal
    keys inside the candidate band, all staged by that one wave."""
    rng = np.random.default_rng(seed)
    g = rng.standard_normal(n).astype(np.float32)
    r = np.zeros(n, dtype=np.float32) if res is None else res
    sub = _wave_share(chunk, wave)
    assert sub.size == CHUNK // 4 and abs(sub.size - 0.05 * n) < 0.001 * n and sub.max() < n
    t = O.residual_compensate(g, None if res is None else res, beta, gamma).ravel()
    rest = np.ones(n, dtype=bool)
    rest[sub] = False
    k = O.ratio_k(n, ratio)
    kth = np.sort(np.abs(t[rest]))[::-1][k - 1]
    # four floats under the k-th magnitude: gamma * g + beta * r is c on the subset wherever the f32
    # rounding allows (everywhere without a residual) and within a float or two of it elsewhere
    c = np.float32(kth)
    for _ in range(4):
        c = np.nextafter(c, np.float32(0))
    g[sub] = ((c - np.float32(beta) * r[sub]) / np.float32(gamma)).astype(np.float32)
    return g, sub, c


@functools.lru_cache(maxsize=None)
def _oracle(n, kinds, seed, ratio=0.01, beta=1.0, gamma=1.0):
    """One name's sequence by the oracle, computed once and shared (read-only):
    [(gradient, residual after, dense output, payload values sorted by index, sorted indices)].
    Kinds: test_gpu_out_lines._gradient's, and ("band", chunk, wave)."""
    res, steps = None, []
    for s, kind in enumerate(kinds):
        if isinstance(kind, tuple):
            g, sub, c = _band_gradient(n, seed + s, res, ratio, beta, gamma, kind[1], kind[2])
        else:
            g = _gradient(n, kind, seed + s, res)
        t, vals, idx, res, out = O.topk_residual_step(g, res, ratio, beta=beta, gamma=gamma)
        if isinstance(kind, tuple):
            # more equal keys than the wave's list region holds, every one of them below the k-th key
            assert int((np.abs(t[sub]) == c).sum()) > LIST_WAVE
            assert c < np.abs(vals).min() and np.abs(t[sub]).max() < np.abs(vals).min()
        order = np.argsort(idx, kind="stable")
        step = (g, res, out, np.asarray(vals)[order], np.asarray(idx)[order].astype(np.int64))
        for a in step:
            a.setflags(write=False)
        steps.append(step)
    return steps


class _StepsPayload(_Steps):
    """_Steps (take(dense=True) -> ops.topk_residual_step -> keep: the line map is live), keeping the
    step's payload too."""

    def step(self, tensor, name):
        ops = self.ops
        g = ops.dev_f32(tensor)
        k = ops.ratio_k(g.numel(), self.ratio)
        res = self.memory.residuals.get(name)
        has = res is not None
        if not has:
            res = torch.empty_like(g)
        out, _ = self.compressor._recycler.take(name, g, dense=True)
        _, vals, idx = ops.topk_residual_step(g, res, has, self.beta, self.gamma, k, out=out)
        self.memory.residuals[name] = res
        self.compressor._recycler.keep(name, out, idx)
        self.payload = (vals, idx)
        return out.view(tensor.shape)


def _sorted_payload(vals, idx):
    v, i = _np(vals), _np(idx).astype(np.int64)
    order = np.argsort(i, kind="stable")
    return v[order], i[order]


def _shifted(a):
    """a on the device as a view offset by one element: 4-B aligned only."""
    base = torch.zeros(a.size + 1, device=DEV)
    base[1:].copy_(_t(a))
    return base[1:]


@functools.lru_cache(maxsize=None)
def _gpu(n, kinds, seed, limit, ratio=0.01, beta=1.0, gamma=1.0, align="aligned"):
    """The sequence on the GPU under grid limit `limit`: [(residual, output, values, indices)] as host
    arrays, and the line map's validity word after every step (None without a map).
    align "g": the gradient is a view offset by one element; "all": residual and output too (the
    ops-level step with its own line map: the recycler only ever hands out whole allocations)."""
    from grace_amd import ops
    ops.topk_main_grid_limit(limit)
    seq = _oracle(n, kinds, seed, ratio, beta, gamma)
    got, valid = [], []
    if align == "all":
        k = ops.ratio_k(n, ratio)
        res = torch.zeros(n + 1, device=DEV)[1:]
        out = torch.full((n + 1,), float("nan"), device=DEV)[1:]
        lines = ops.topk_lines_map(n, out.device)
        for s, step in enumerate(seq):
            _, vals, idx = ops.topk_residual_step(_shifted(step[0]), res, s > 0, beta, gamma, k, out=out,
                                                  lines=lines if s > 0 else None)
            got.append((_np(res), _np(out)) + _sorted_payload(vals, idx))
            valid.append(int(lines[0]))
    else:
        comm = _StepsPayload(ratio, beta, gamma)
        for step in seq:
            out = comm.step(_shifted(step[0]) if align == "g" else _t(step[0]), "b")
            got.append((_np(comm.memory.residuals["b"]), _np(out)) + _sorted_payload(*comm.payload))
            del out
            lines = _map_of(comm, "b")
            valid.append(None if lines is None else int(lines[0]))
        assert comm.compressor._recycler.dense_hits == len(seq) - 1   # the kept buffer came back every time
    ops.topk_main_grid_limit(0)
    return got, valid


def _check(n, kinds, seed, limit, **kw):
    seq = _oracle(n, kinds, seed, kw.get("ratio", 0.01), kw.get("beta", 1.0), kw.get("gamma", 1.0))
    got, valid = _gpu(n, kinds, seed, limit, **kw)
    base, _ = _gpu(n, kinds, seed, 0, **kw)
    for s, (step, g, b) in enumerate(zip(seq, got, base)):
        assert same_bits(g[1], step[2]), ("out", s)
        assert same_bits(g[0], step[1]), ("residual", s)
        assert np.array_equal(g[3], step[4]) and same_bits(g[2], step[3]), ("payload", s)
        for x, y in zip(g, b):                                 # ... and the default grid's result
            assert same_bits(x, y), ("default grid", s)
    return valid


@pytest.mark.parametrize("limit", LIMITS)
@pytest.mark.parametrize("n", SIZES)
def test_every_size_under_every_grid(n, limit):
    valid = _check(n, NORMAL4, 1100, limit)
    assert valid == [None, 1, 1, 1]        # no map on the name's first step, a valid one after every later step


@pytest.mark.parametrize("limit", LIMITS)
@pytest.mark.parametrize("align", ["g", "all"])
def test_misaligned_buffers(align, limit):
    """Every chunk is off the fast path, under a workgroup that takes several."""
    _check(36869, NORMAL4, 1200, limit, align=align)


@pytest.mark.parametrize("limit", LIMITS)
@pytest.mark.parametrize("n", [36869, 61440])
def test_non_unit_factors(n, limit):
    _check(n, NORMAL4, 1300, limit, beta=0.9, gamma=1.1)


# (above the candidate list's capacity of 2 k + 65536 entries, so that the ties leave the fast path)
@pytest.mark.parametrize("limit", LIMITS)
@pytest.mark.parametrize("kind", ["const", "zeros"])
def test_exact_fallback_in_the_middle(kind, limit):
    """The exact fallback invalidates the map; the step after it writes every line."""
    valid = _check(100003, ("normal", kind, "normal", "normal"), 1400, limit)
    assert valid == [None, 0, 1, 1]        # invalid after the fallback step, valid again after the next


@pytest.mark.parametrize("limit", LIMITS)
@pytest.mark.parametrize("where", [(0, 3), (2, 1)])
def test_ties_in_the_band_overflow_a_wave_region(where, limit):
    """3,072 equal keys just under the k-th, all in one wave's share of one chunk: the wave's list
    region (512 entries) overflows and the rest leaves entry by entry (spill_entry), whose histogram
    add must not race the workgroup's histogram zeroing -- the first chunk of a workgroup included."""
    kinds = ("normal", ("band",) + where, "normal", ("band",) + where)
    _check(61440, kinds, 1500, limit)


@pytest.mark.parametrize("limit", LIMITS)
def test_first_step_without_residual_then_residual_step(limit):
    """A name's first step has neither residual nor line map (the 12-B pass), the second has both."""
    valid = _check(61443, ("normal", "normal"), 1600, limit)
    assert valid == [None, 1]


def test_limit_is_process_global_and_returns_the_previous():
    from grace_amd import ops
    assert ops.topk_main_grid_limit(3) == 0
    assert ops.topk_main_grid_limit(0) == 3
    assert ops.topk_main_grid_limit(0) == 0
