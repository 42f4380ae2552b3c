"""Line-skipping dense output of the world-1 f32 top-k residual step (DESIGN §4 "Line-skipping
output", grace_topk_residual_step_lines, ops.OUT_LINES): a name's kept output buffer comes back with
its line map, and the main pass stores only the 64-B lines that can be non-zero in this step or
were in the previous one.  Whatever the caller does with its results, every result and residual
must equal the oracle's Allgather(TopK, ResidualMemory).step (grace_dl/dist/compressor/topk.py:32-69,
memory/residual.py:10-20) bit for bit."""
import functools

import numpy as np
import pytest
import torch

from oracle import grace_oracle as O
from tests.golden_util import same_bits

pytestmark = pytest.mark.gpu
DEV = "cuda"
STEPS = 6
# the smallest large-path bucket (all tail), three whole chunks, whole chunks plus a tail, odd sizes
SIZES = [32772, 36864, 36869, 100003, (1 << 20) + 7]


def _np(t):
    return t.detach().cpu().numpy()


def _t(a):
    return torch.from_numpy(a.copy()).to(DEV)      # (the shared oracle arrays are read-only)


class _Memory:
    def __init__(self):
        self.residuals = {}


class _Compressor:
    def __init__(self, recycler):
        self._recycler = recycler


class _Steps:
    """The world-1 residual step exactly as TopKCompressor._fused_step runs it for a bucket that keeps
    its output buffer (take(dense=True) -> ops.topk_residual_step -> keep), without the placement
    probe and at any size: the compressor itself keeps buffers only from ops.PLACE_MIN_N elements
    on, far above the sizes at which the kernels' paths change."""

    def __init__(self, ratio=0.01, beta=1.0, gamma=1.0):
        from grace_amd import ops
        self.ops, self.ratio, self.beta, self.gamma = ops, ratio, beta, gamma
        self.memory = _Memory()
        self.compressor = _Compressor(ops.OutputRecycler())

    def step(self, tensor, name):
        ops = self.ops
        g = ops.dev_f32(tensor)
        k = ops.ratio_k(g.numel(), self.ratio)
        res = self.memory.residuals.get(name)
        has = res is not None
        if not has:
            res = torch.empty_like(g)
        out, _ = self.compressor._recycler.take(name, g, dense=True)
        _, _, idx = ops.topk_residual_step(g, res, has, self.beta, self.gamma, k, out=out)
        self.memory.residuals[name] = res
        self.compressor._recycler.keep(name, out, idx)
        return out.view(tensor.shape)


def _comm(ratio=0.01, beta=1.0, gamma=1.0):
    return _Steps(ratio, beta, gamma)


def _gradient(n, kind, seed, res):
    """kind "zeros" / "const": the gradient that makes the COMPENSATED bucket t = r + g 99.75 % exact
    zeros / (almost everywhere) one constant -- massive ties at the k-th key, so the exact fallback runs."""
    rng = np.random.default_rng(seed)
    r = np.zeros(n, dtype=np.float32) if res is None else res
    if kind == "const":
        return (np.float32(0.5) - r).astype(np.float32)      # r + (0.5 - r) rounds to 0.5 almost everywhere
    g = rng.standard_normal(n).astype(np.float32)
    if kind == "zeros":
        z = rng.random(n) < 0.9975
        g[z] = -r[z]                                         # r + (-r) is exactly +0
    return g


@functools.lru_cache(maxsize=None)
def _oracle(n, kinds, seed, ratio=0.01, beta=1.0, gamma=1.0):
    """The oracle's sequence for one name, computed once and shared (read-only):
    [(gradient, residual after, dense output)]."""
    res, steps = None, []
    for s, kind in enumerate(kinds):
        g = _gradient(n, kind, seed + s, res)
        _, _, _, res, out = O.topk_residual_step(g, res, ratio, beta=beta, gamma=gamma)
        for a in (g, res, out):
            a.setflags(write=False)
        steps.append((g, res, out))
    return steps


NORMAL = ("normal",) * STEPS


def _check(comm, name, step, s, out):
    g, res, exp = step
    assert same_bits(_np(out), exp), (name, s)
    assert same_bits(_np(comm.memory.residuals[name]), res), (name, s)


def _map_of(comm, name):
    ent = comm.compressor._recycler._hit.get(name)
    return None if ent is None else ent[6]


@pytest.mark.parametrize("n", SIZES)
def test_dropped_results_every_size(n):
    comm = _comm()
    for s, step in enumerate(_oracle(n, NORMAL, 100)):
        out = comm.step(_t(step[0]), "b")
        _check(comm, "b", step, s, out)
        del out
    rec = comm.compressor._recycler
    assert rec.dense_hits == STEPS - 1 and rec.hits == 0
    lines = _map_of(comm, "b")
    assert lines is not None and int(lines[0]) == 1      # the mode ran and the last step left a valid map


def test_map_marks_fewer_than_all_lines():
    """randn at ratio 0.01: the map after a step marks well under all lanes of the whole chunks --
    the mode really skips (a flagged share of ~1.3 % dirties about a fifth of the 64-B lines)."""
    n = (1 << 20) + 7
    comm = _comm()
    for s, step in enumerate(_oracle(n, NORMAL, 100)[:3]):
        out = comm.step(_t(step[0]), "b")
        del out
    words = _np(_map_of(comm, "b")).view(np.uint64)
    assert int(words[0]) == 1
    body = words[16:]
    whole = n // 12288 * 48                              # the words of the whole chunks
    assert body.size == (n + 12287) // 12288 * 48
    marked = int(np.unpackbits(body[:whole].view(np.uint8)).sum())
    assert 0 < marked < 0.5 * 64 * whole
    assert np.all(body[whole:] == np.uint64(0xFFFFFFFFFFFFFFFF))   # the tail chunk stores densely


@pytest.mark.parametrize("form", ["view", "factors", "k1", "ratio03"])
def test_input_forms(form):
    n = 36869
    ratio = {"k1": 1e-9, "ratio03": 0.3}.get(form, 0.01)
    beta, gamma = (0.9, 0.5) if form == "factors" else (1.0, 1.0)
    comm = _comm(ratio, beta, gamma)
    for s, step in enumerate(_oracle(n, NORMAL, 200, ratio, beta, gamma)):
        if form == "view":                    # g[1:]: 4-B aligned only, the guarded path
            base = torch.zeros(n + 1, device=DEV)
            base[1:].copy_(_t(step[0]))
            g = base[1:]
        else:
            g = _t(step[0])
        out = comm.step(g, "b")
        _check(comm, "b", step, s, out)
        del out
    assert comm.compressor._recycler.dense_hits == STEPS - 1
    assert _map_of(comm, "b") is not None


def test_held_results_are_never_reused_or_changed():
    n = 100003
    comm = _comm()
    held = []
    for s, step in enumerate(_oracle(n, NORMAL, 300)):
        out = comm.step(_t(step[0]), "b")
        _check(comm, "b", step, s, out)
        held.append(out)
        del out
    assert comm.compressor._recycler.dense_hits == 0
    assert len({t.data_ptr() for t in held}) == STEPS
    for s, (t, step) in enumerate(zip(held, _oracle(n, NORMAL, 300))):
        assert same_bits(_np(t), step[2]), s


def test_result_edited_in_place_then_dropped():
    n = 100003
    comm = _comm()
    ptrs = []
    for s, step in enumerate(_oracle(n, NORMAL, 300)):
        out = comm.step(_t(step[0]), "b")
        _check(comm, "b", step, s, out)
        ptrs.append(out.data_ptr())
        if s in (1, 3):
            out.add_(1.0)                     # every zero of the kept buffer gone
        del out
    assert comm.compressor._recycler.dense_hits == STEPS - 1 - 2   # the edited ones were not handed back


def test_two_names_interleaved_and_two_streams():
    n = 36869
    comm = _comm()
    seqs = [_oracle(n, NORMAL, 400), _oracle(n, NORMAL, 500)]
    streams = [torch.cuda.Stream() for _ in range(2)]
    for s in range(STEPS):
        outs = []
        for j in range(2):
            with torch.cuda.stream(streams[j]):
                outs.append(comm.step(_t(seqs[j][s][0]), f"b{j}"))
        torch.cuda.synchronize()
        for j in range(2):
            _check(comm, f"b{j}", seqs[j][s], s, outs[j])
        del outs
    assert comm.compressor._recycler.dense_hits == 2 * (STEPS - 1)
    # one stream, the names interleaved
    comm = _comm()
    for s in range(STEPS):
        for j in range(2):
            out = comm.step(_t(seqs[j][s][0]), f"b{j}")
            _check(comm, f"b{j}", seqs[j][s], s, out)
            del out


# (sizes above the candidate list's capacity of 2 k + 65536 entries: below it a bucket of ties fits
# the list and stays on the fast path, with every line marked)
@pytest.mark.parametrize("n", [100003, (1 << 20) + 7])
def test_exact_fallback_in_the_middle_invalidates_the_map(n):
    from grace_amd import ops
    kinds = ("normal", "normal", "zeros", "normal", "normal", "const", "normal", "normal")
    comm = _comm()
    k = ops.ratio_k(n, 0.01)
    for s, step in enumerate(_oracle(n, kinds, 600)):
        out = comm.step(_t(step[0]), "b")
        torch.cuda.synchronize()
        status = ops.topk_status(n, k, torch.device(DEV, 0))
        _check(comm, "b", step, s, out)
        del out
        lines = _map_of(comm, "b")
        if s >= 1:
            # the validity word follows the path the step took: a fallback step leaves the map
            # invalid, so the step after it writes every line and leaves it valid again
            assert int(lines[0]) == (1 if status == 0 else 0), (s, status)
        if kinds[s] != "normal":
            assert status == 1, s                             # the exact fallback ran
    assert comm.compressor._recycler.dense_hits == len(kinds) - 1


def test_switch_toggled_mid_sequence(monkeypatch):
    from grace_amd import ops
    n = 100003
    comm = _comm()
    ptrs = set()
    for s, step in enumerate(_oracle(n, NORMAL + NORMAL[:2], 700)):
        monkeypatch.setattr(ops, "OUT_LINES", s not in (3, 4, 6))
        out = comm.step(_t(step[0]), "b")
        _check(comm, "b", step, s, out)
        if s >= 1:
            ptrs.add(out.data_ptr())
        del out
        assert (_map_of(comm, "b") is not None) == (s >= 1 and ops.OUT_LINES), s   # off: the map is dropped
    assert len(ptrs) == 1                                  # the same kept buffer throughout
    assert comm.compressor._recycler.dense_hits == STEPS + 2 - 1


def _allgather(recycle=True):
    from grace_amd.dist.communicator.allgather import Allgather
    from grace_amd.dist.compressor.topk import TopKCompressor
    from grace_amd.dist.memory.residual import ResidualMemory
    return Allgather(TopKCompressor(0.01, recycle_output=recycle), ResidualMemory(), 1)


def test_allgather_step_uses_the_map_on_a_placed_bucket():
    """Allgather(TopK, ResidualMemory, 1).step itself, at the smallest size whose buffer it keeps:
    the map arrives with the kept buffer without the compressor naming it."""
    from grace_amd import ops
    n = ops.PLACE_MIN_N + 4096
    comm = _allgather()
    for s, step in enumerate(_oracle(n, NORMAL[:4], 800)):
        out = comm.step(_t(step[0]), "b")
        _check(comm, "b", step, s, out)
        del out
        lines = _map_of(comm, "b")
        assert (lines is not None) == (s >= 1), s
    rec = comm.compressor._recycler
    assert rec.dense_hits == 3 and rec.hits == 0
    words = _np(lines).view(np.uint64)
    assert int(words[0]) == 1
    assert 0 < int(np.unpackbits(words[16:].view(np.uint8)).sum()) < 0.5 * 64 * (words.size - 16)


def test_recycle_output_false_keeps_nothing():
    from grace_amd import ops
    n = ops.PLACE_MIN_N
    comm = _allgather(recycle=False)
    for s, step in enumerate(_oracle(n, NORMAL[:2], 900)):
        out = comm.step(_t(step[0]), "b")
        _check(comm, "b", step, s, out)
        del out
    rec = comm.compressor._recycler
    assert rec.dense_hits == 0 and rec.hits == 0 and not rec._hit


def test_a_map_never_follows_another_tensor():
    """The hand-off is by tensor identity: a step whose output is not the tensor the recycler has just
    handed back gets no map, and nothing is kept beside a buffer the step did not write with one."""
    from grace_amd import ops
    n = 36869
    k = ops.ratio_k(n, 0.01)
    seq = _oracle(n, NORMAL, 200)
    rec = ops.OutputRecycler()
    res = torch.empty(n, device=DEV)
    out, _ = rec.take("b", res, dense=True)
    ops.topk_residual_step(_t(seq[0][0]), res, False, 1.0, 1.0, k, out=out)
    rec.keep("b", out, None)
    del out
    for s in (1, 2, 3):
        out, _ = rec.take("b", res, dense=True)           # a hit: the note names this tensor
        other = torch.full((n,), float("nan"), device=DEV)
        ops.topk_residual_step(_t(seq[s][0]), res, True, 1.0, 1.0, k, out=other)   # ... but the step writes another
        assert same_bits(_np(other), seq[s][2]), s        # every line written: no map was used
        rec.keep("b", out, None)
        assert rec._hit["b"][6] is None
        del out, other


@pytest.mark.parametrize("n", [36869, (1 << 20) + 7])
def test_first_step_on_a_nan_filled_buffer_writes_every_line(n):
    """ops level: a buffer full of NaN with a fresh (invalid) map -- the first step writes every
    line; the following steps skip on the same buffer and map."""
    from grace_amd import ops
    k = ops.ratio_k(n, 0.01)
    seq = _oracle(n, NORMAL, 100 if n > 36869 else 200)
    out = torch.full((n,), float("nan"), device=DEV)
    lines = ops.topk_lines_map(n, out.device)
    assert lines is not None and int(lines[0]) == 0
    res = _t(seq[0][1])      # the residual after step 0
    for s in range(1, STEPS):
        g = _t(seq[s][0])
        ops.topk_residual_step(g, res, True, 1.0, 1.0, k, out=out, lines=lines)
        assert same_bits(_np(out), seq[s][2]), s
        assert same_bits(_np(res), seq[s][1]), s
        assert int(lines[0]) == 1, s


def test_lines_argument_errors():
    from grace_amd import ops
    n = 36869
    g = torch.zeros(n, device=DEV)
    res = torch.zeros(n, device=DEV)
    lines = ops.topk_lines_map(n, g.device)
    with pytest.raises(ValueError):
        ops.topk_residual_step(g, res, True, 1.0, 1.0, 8, out=None, lines=lines)
    with pytest.raises(ops._lib.GraceNativeError):       # a map too short for the bucket
        ops.topk_residual_step(g, res, True, 1.0, 1.0, 8, out=torch.zeros(n, device=DEV), lines=lines[:32])
    assert ops.topk_lines_map(ops.TOPK_SMALL_N, g.device) is None
