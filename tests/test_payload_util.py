"""The host reference and payload builders of the sparse-decode tests, checked on the CPU."""
import numpy as np
import pytest

from oracle import grace_oracle as O
from tests import payload_util as U


def _dense(touched, vals, n):
    out = np.zeros(n, dtype=np.float32)
    out[touched] = vals
    return out


@pytest.mark.parametrize("divisor", [1, 3, 4])
def test_ref_aggregate_equals_python_sum_of_dense_decodes(divisor):
    n = 40
    idx = [np.array([3, 0, 17, 39, 8], np.int32), np.array([17, 3, 5, 8], np.int32), np.zeros(0, np.int32),
           np.array([8, 39, 3, 17, 0, 21], np.int32)]
    vals = [np.array([-0.0, 1.5, 1e-3, -0.0, 3e7], np.float32), np.array([np.nan, -0.0, 2.25, 1.0], np.float32),
            np.zeros(0, np.float32), np.array([-3e7, -0.0, 1e-9, 7.0, -1.5, -0.0], np.float32)]
    pay = list(zip(vals, idx))
    exp = O.python_sum([O.sparse_decode(v, i, n) for v, i in pay])
    if divisor != 1:
        exp = (exp / np.float32(divisor)).astype(np.float32)
    touched, got = U.ref_aggregate(pay, n, divisor)
    assert np.array_equal(touched, np.unique(np.concatenate(idx)))
    assert np.array_equal(U.bits(_dense(touched, got, n)), U.bits(exp))
    assert np.isnan(exp[17]) and U.bits(exp)[39] == 0 and U.bits(exp)[21] == 0     # NaN kept, -0.0 -> +0.0


def test_group_on_host_wire_form():
    rng = np.random.default_rng(3)
    n, k = 5 * U.CHUNK + 7, 1001                                        # odd k: one u16 of padding
    idx = rng.choice(n, k, replace=False).astype(np.int32)
    vals = U.draw_values(rng, k)
    w = U.group_on_host(vals, idx, n, seed=1)
    nch, ow = 6, (k + 1) // 2
    assert w.dtype == np.uint32 and w.size == k + ow + nch
    offs = w[k:k + ow].view(np.uint16)
    ends = w[k + ow:]
    assert offs[k] == 0 and np.all(offs < U.CHUNK)
    assert np.array_equal(np.diff(ends, prepend=0), np.bincount(idx >> 13, minlength=nch)) and ends[-1] == k
    back = np.searchsorted(ends, np.arange(k), side="right") * U.CHUNK + offs[:k]
    o1, o2 = np.argsort(back), np.argsort(idx)
    assert np.array_equal(back[o1], idx[o2]) and np.array_equal(w[:k][o1], U.bits(vals)[o2])
    assert not np.array_equal(back, np.sort(idx))                       # shuffled inside the chunks
    w2 = U.group_on_host(vals, idx, n, seed=2)
    assert not np.array_equal(w, w2) and np.array_equal(w[k + ow:], w2[k + ow:])


def test_build_ranks_follows_the_table():
    for world, n in ((9, U.BASE_N), (9, 6 * U.CHUNK), (65, U.BASE_N)):
        ranks = U.sorted_base_case(world, n)
        last = (n - 1) >> 13
        k = ranks[0][1].size
        for w, (v, i) in enumerate(ranks):
            assert i.size == k == v.size and np.unique(i).size == k and i.min() >= 0 and i.max() < n
            per = np.bincount(i >> 13, minlength=last + 1)
            assert per[0] == U._COUNTS[w % 8] and per[2] == U._COUNTS[(w + 3) % 8]
            if last == 6:
                assert per[6] == w % 6 and per[5] == 0
            else:
                assert per[5] == w % 6
            assert np.isnan(v).sum() == 1 and (U.bits(v) == 0x80000000).sum() >= 3
        seen = {int(c) for _, i in ranks for c in np.bincount(i >> 13, minlength=last + 1)[[0, 2]]}
        assert seen >= set(U._COUNTS)


def test_padded_buffers_hold_poison_at_index_zero():
    for counts in U.SCATTER_COUNTS:
        ranks, vals, idx = U.scatter_case(counts)
        for w, c in enumerate(counts):
            assert np.all(idx[w, c:] == 0) and np.all(vals[w, c:] == U.POISON) and c < U.SCATTER_STRIDE
            assert np.array_equal(idx[w, :c], ranks[w][1]) and ranks[w][1].size == c
    for counts in U.CAPPED_COUNTS:
        ranks, recs = U.capped_case(counts)
        for w, c in enumerate(counts):
            live = min(c, U.CAP)
            assert tuple(recs[w, :4]) == (c, U.CAP, 0, 0) and ranks[w][1].size == live
            assert np.all(recs[w, 4 + U.CAP + live:] == 0)
            assert np.all(recs[w, 4 + live:4 + U.CAP].view(np.float32) == U.POISON)
    assert {c for cs in U.CAPPED_COUNTS for c in cs} == {0, 1, 999, 1000, 1001, 5000}


def test_every_case_of_three_ranks_or_more_can_catch_an_order_bug():
    """Reversing the ranks changes at least one bit of the aggregate in every case that three or more
    ranks with entries take part in.  With entries from two ranks only -- the scatter cases where one
    of three ranks is empty -- (0 + a) + b and (0 + b) + a are the same f32, so no input could tell
    the orders apart; that is asserted as well, so the exception is a checked one."""
    names = []
    for name, payloads, n in U.order_cases():
        names.append(name)
        assert len(payloads) >= 3
        live = sum(1 for _, i in payloads if i.size)
        assert U.order_matters(payloads, n) == (live >= 3), name
    assert len(names) == len(set(names)) and len(names) >= 14
