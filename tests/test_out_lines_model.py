"""CPU model of the line-skipping dense output of the world-1 top-k residual step (DESIGN §4
"Line-skipping output", grace_topk_residual_step_lines), run against the oracle's
Allgather(TopK, ResidualMemory).step sequence.

The protocol, as the kernels implement it:
  * flagged   = the elements whose key |t| is at or above the step's lower threshold `lo` (a superset
                of the selection: the sure elements and every candidate);
  * dirty     = a line with a flagged element in this step;
  * written   = the lines the main pass stores: dirty now or dirty in the buffer's previous step --
                every line when the map is invalid or missing;
  * a written line receives the PROVISIONAL dense output (0 + t above the provisional threshold
                `mid`, else +0); the finalize then fixes single elements, at flagged positions only;
  * a step off the fast path (exact fallback) rewrites the buffer wherever it likes and marks the
                map invalid; a miss (result held or edited) gets a fresh buffer and no map.
Invariant: after a step, every line the step's map does not mark dirty holds +0 bits throughout.
The model asserts, after every step, that its buffer equals the oracle's dense output bit for bit
and that the invariant holds -- for 64-B and 128-B lines, with ties, all-zero gradients, fallback
steps and misses in the sequence."""
import functools

import numpy as np
import pytest

from oracle import grace_oracle as O
from tests.golden_util import same_bits

N = 36864            # three whole chunks of the main pass
RATIO = 0.01
BAND = 0.0123        # the bracket's lower threshold sits near rank 1.23 % for k = 1 %


def _keys(t):
    return t.view(np.uint32) & np.uint32(0x7FFFFFFF)


class KeptOutput:
    """One name's kept output buffer with its line map, and the protocol's three kinds of step."""

    def __init__(self, n, line):
        self.n, self.line = n, line
        self.nlines = (n + line - 1) // line
        self.buf = None          # the kept buffer (None: nothing kept yet)
        self.dirty = None        # the map: one flag per line (None: no map beside the buffer)
        self.valid = False       # the map's validity word
        self.full_writes = 0
        self.skipped_lines = 0

    def _line_any(self, flags):
        pad = np.zeros(self.nlines * self.line, dtype=bool)
        pad[:self.n] = flags
        return pad.reshape(self.nlines, self.line).any(axis=1)

    def miss(self, rng):
        """The caller held or edited the result: a fresh buffer (garbage) and no map."""
        self.buf = rng.standard_normal(self.n).astype(np.float32)
        self.buf[::7] = np.nan
        self.dirty, self.valid = None, False

    def step_fast(self, t, sel_idx, lo, mid, with_map):
        """A step on the sampled fast path.  with_map False: the plain dense step (a miss's first
        step: every element written, no map left)."""
        keys = _keys(t)
        flagged = keys >= lo
        prov = np.where(keys > mid, np.float32(0) + t, np.float32(0)).astype(np.float32)
        if not with_map:
            self.buf[:] = prov
            self.full_writes += 1
        else:
            if self.dirty is None:                      # first hit of a kept buffer: a fresh, invalid map
                self.dirty, self.valid = np.zeros(self.nlines, dtype=bool), False
            now = self._line_any(flagged)
            written = (now | self.dirty) if self.valid else np.ones(self.nlines, dtype=bool)
            if not self.valid:
                self.full_writes += 1
            self.skipped_lines += int((~written).sum())
            w_el = np.repeat(written, self.line)[:self.n]
            self.buf[w_el] = prov[w_el]
            self.dirty = now                            # in place: each wave rewrites its own words
            self.valid = True                           # the finalize, fast path
        # the finalize's fix-ups: single elements whose provisional decision was wrong -- all of them
        # candidates, hence flagged
        selected = np.zeros(self.n, dtype=bool)
        selected[sel_idx] = True
        fix = selected != (keys > mid)
        assert not (fix & ~flagged).any(), "a fix-up outside the flagged set"
        assert not (selected & ~flagged).any(), "a selected element below the lower threshold"
        self.buf[fix] = np.where(selected[fix], np.float32(0) + t[fix], np.float32(0))

    def step_fallback(self, out, rng):
        """A step off the fast path: the buffer is rewritten arbitrarily (here: garbage first, then
        the result everywhere), the map's words are whatever the main pass left, the word says invalid."""
        self.buf[:] = rng.standard_normal(self.n).astype(np.float32)
        self.buf[:] = out
        if self.dirty is not None:
            self.dirty = rng.random(self.nlines) < 0.5
        self.valid = False

    def check_invariant(self):
        if self.dirty is None or not self.valid:
            return
        clean = np.repeat(~self.dirty, self.line)[:self.n]
        assert not self.buf.view(np.uint32)[clean].any(), "a line not marked dirty holds a non-zero bit pattern"


def _gradient(rng, kind, n):
    if kind == "zeros":
        return np.zeros(n, dtype=np.float32)
    if kind == "ties":
        # 1.5 % of the elements at three magnitudes far above the residual's ulp, both signs: t = r + g
        # rounds to them exactly, so the k-th largest sits inside a run of equal keys (lowest index wins)
        g = np.zeros(n, dtype=np.float32)
        i = rng.choice(n, n * 3 // 200, replace=False)
        g[i] = (rng.integers(1, 4, i.size) * rng.choice([-1.0, 1.0], i.size) * 2.0 ** 30).astype(np.float32)
        return g
    if kind == "sparse":         # 99.75 % zeros
        g = np.zeros(n, dtype=np.float32)
        i = rng.choice(n, n // 400, replace=False)
        g[i] = rng.standard_normal(i.size).astype(np.float32)
        return g
    return rng.standard_normal(n).astype(np.float32)


def _thresholds(t, k):
    """(lo, mid, fast): the band a sampled bracket would publish -- lo at rank BAND * n, mid between
    lo and the k-th key -- and whether the step stays on the fast path (the band is not degenerate:
    lo > 0 and the flagged set is no more than twice the band)."""
    keys = np.sort(_keys(t))[::-1]
    lo = int(keys[min(t.size - 1, int(BAND * t.size))])
    kth = int(keys[k - 1])
    mid = (lo + kth) // 2        # lo <= mid <= kth: nothing above mid is below the band
    flagged = int((_keys(t) >= lo).sum())
    fast = lo > 0 and flagged <= 2 * int(BAND * t.size) + 64
    return np.uint32(lo), np.uint32(mid), fast


KINDS = tuple(["normal"] * 6 + ["ties", "normal", "zeros", "normal", "normal", "sparse"] + ["normal"] * 4 +
              ["ties", "normal", "normal", "zeros", "zeros", "normal", "normal", "normal"])


@functools.lru_cache(maxsize=None)
def _sequence(kinds, seed):
    """The oracle's step sequence, computed once and shared: per step (t, payload indices, out,
    lo, mid, fast)."""
    rng = np.random.default_rng(seed)
    k = O.ratio_k(N, RATIO)
    res, steps = None, []
    for kind in kinds:
        g = _gradient(rng, kind, N)
        t, _, idx, res, out = O.topk_residual_step(g, res, RATIO)
        t = np.ascontiguousarray(t, dtype=np.float32)
        for a in (t, out):
            a.setflags(write=False)
        steps.append((t, np.asarray(idx, dtype=np.int64), out) + _thresholds(t, k))
    return steps


@pytest.mark.parametrize("line", [16, 32])   # elements per line: 64 B (4 lanes) and 128 B (8 lanes)
def test_line_map_protocol_matches_the_oracle(line):
    rng = np.random.default_rng(4100 + line)
    kinds = KINDS
    miss_at = {0, 5, 14, 15}          # the result was held / edited before these steps
    forced_fallback = {3, 9, 18, 21}  # steps that leave the fast path (bracket miss, list overflow)
    assert len(kinds) >= 20
    kept = KeptOutput(N, line)
    n_fast_map = n_fallback = 0
    for s, (kind, (t, idx, out, lo, mid, fast)) in enumerate(zip(kinds, _sequence(kinds, 4100))):
        missed = s in miss_at or kept.buf is None
        if missed:
            kept.miss(rng)
        if fast and s not in forced_fallback:
            kept.step_fast(t, idx, lo, mid, with_map=not missed)
            n_fast_map += not missed
        else:
            kept.step_fallback(out, rng)
            n_fallback += 1
        assert same_bits(kept.buf, out), (s, kind)
        kept.check_invariant()
    assert n_fallback >= 4 and n_fast_map >= 10
    # the mode really skips, and every miss, first hit and post-fallback step wrote in full
    assert kept.skipped_lines > 0
    assert kept.full_writes >= len(miss_at)


@pytest.mark.parametrize("line", [16, 32])
def test_line_map_needs_the_previous_steps_lines(line):
    """The store rule's second half: with only "dirty now" written, the previous step's picks
    survive in the buffer -- the model must catch that (it guards the test above against a vacuous
    pass)."""
    rng = np.random.default_rng(7)
    kept = KeptOutput(N, line)
    stale = False
    for t, idx, out, lo, mid, fast in _sequence(KINDS, 4100)[:4]:
        assert fast
        if kept.buf is None:
            kept.miss(rng)
            kept.step_fast(t, idx, lo, mid, with_map=False)
            continue
        if kept.valid:
            kept.dirty[:] = False     # forget the previous step's lines
        kept.step_fast(t, idx, lo, mid, with_map=True)
        stale = stale or not same_bits(kept.buf, out)
    assert stale
