"""CPU checks of the inputs tests/test_gpu_dgc_edges.py drives the DGC engine with: each one takes
the oracle's adjustment loop (oracle/grace_oracle.py dgc_compress) down the path it was built for."""
import numpy as np
import pytest

from oracle import grace_oracle as O
from tests.dgc_edge_util import LOOP_CASES, N, RATIO, ns_of


@pytest.mark.parametrize("name", sorted(LOOP_CASES))
def test_loop_case_takes_its_path(name):
    case = LOOP_CASES[name]()
    trace = case.check_path()
    # the trace is dgc_compress's own loop: same final threshold, same selection
    vals, idx, mask, thr = O.dgc_compress(case.x, case.sidx, case.ratio)
    assert np.array_equal(np.asarray(thr).view(np.uint32), np.asarray(trace[-1][1]).view(np.uint32))
    assert idx.size == int(mask.sum()) == trace[-1][2] and len(trace) <= 11
    assert [m for m, _, _ in trace[1:]] == list(O.dgc_adjust_path(case.x, case.sidx, case.ratio))


def test_adjust_path_replays_the_loop():
    """The path's moves applied to the sampled threshold in f32 give dgc_compress's threshold."""
    rng = np.random.default_rng(3)
    x = rng.standard_normal(N).astype(np.float32)
    sidx = np.full(ns_of(N), int(np.argmax(np.abs(x))))
    path = O.dgc_adjust_path(x, sidx, RATIO)
    assert path and path[0] == "D"
    thr = np.abs(x).max()
    for move in path:
        thr = np.float32(np.float32(1.3 if move == "U" else 0.7) * thr)
    assert thr == O.dgc_compress(x, sidx, RATIO)[3]
