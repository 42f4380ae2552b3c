"""tests/shard_select_util.py on the CPU: ref_select against a brute-force Python sort, branch_model
against hand-counted records, and -- for every builder / parameter pair the GPU tests run
(tests/test_gpu_shard_select_cases.py) -- that the model reports the branch the case is named
after.  The last is what keeps a GPU case from silently missing its branch."""
import numpy as np
import pytest

from tests import shard_select_util as U

POOL = np.array([0x00000000, 0x80000000, 0x3F800000, 0xBF800000, 0x3F800001, 0x3F800200, 0x40000000, 0xC0000000,
                 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00001, 0x7F800001, 0x00000001, 0x80000001, 0x3F000000],
                dtype=np.uint32)


def _brute(vals, li, sizes, bases, hdr, k, rank, out_base, out_len):
    world, cap = vals.shape
    ents = []
    for w in range(world):
        for j in range(cap):
            if li[w, j] >= 0:
                ents.append((-(int(vals[w, j]) & 0x7FFFFFFF), int(bases[w]) + int(li[w, j]), w, j))
    ents.sort()
    picked = {(w, j) for _, _, w, j in ents[:k]}
    sel_gi = np.full((world, cap), -1, dtype=np.int32)
    out = np.zeros(out_len, dtype=np.float32)
    rest = []
    for _, gi, w, j in ents:
        if (w, j) in picked:
            sel_gi[w, j] = gi
            if out_base <= gi < out_base + out_len:
                with np.errstate(invalid="ignore"):
                    out[gi - out_base] = np.float32(0.0) + vals[w:w + 1, j].view(np.float32)[0]
        elif w == rank:
            rest.append((int(li[w, j]), int(vals[w, j])))
    status = (1 if any(int(hdr[w]) != int(sizes[w]) for w in range(world)) else 0) | (2 if len(ents) < k else 0)
    return sel_gi, out, sorted(rest), status


def test_ref_select_against_a_brute_force_sort():
    rng = np.random.default_rng(5)
    for case in range(300):
        world, cap = int(rng.integers(1, 5)), int(rng.integers(1, 7))
        sizes = [int(rng.integers(cap, cap + 4)) for _ in range(world)]
        bases = U.bases_of(sizes)
        vals = POOL[rng.integers(0, POOL.size, (world, cap))]
        li = np.full((world, cap), -1, dtype=np.int32)
        for w in range(world):
            m = int(rng.integers(0, cap + 1))
            li[w, :m] = rng.permutation(sizes[w])[:m]
        valid = int((li >= 0).sum())
        k = int(rng.integers(1, valid + 3))
        rank = int(rng.integers(0, world))
        hdr = list(sizes)
        if case % 7 == 0:
            hdr[int(rng.integers(0, world))] += 1
        n = sum(sizes)
        out_base = int(rng.integers(0, n))
        out_len = int(rng.integers(0, n - out_base + 1))
        got = U.ref_select(vals, li, sizes, bases, hdr, k, rank, out_base, out_len)
        sel_gi, out, rest, status = _brute(vals, li, sizes, bases, hdr, k, rank, out_base, out_len)
        assert np.array_equal(got["sel_gi"], sel_gi.ravel()), case
        assert np.array_equal(got["sel"], sel_gi >= 0)
        assert np.array_equal(got["pay_idx"], sel_gi[rank])
        assert np.array_equal(got["out_f32"].view(np.uint32), out.view(np.uint32)), case
        assert sorted(zip(got["restore"][0].tolist(), got["restore"][1].tolist())) == rest
        assert got["status"] == status
        assert int(got["sel"].sum()) == min(k, valid)


def test_ref_select_writes_plus_zero_and_keeps_nan_payloads():
    vals = np.array([[0x80000000, 0xFFC12345, 0x7F800001, 0xBF800000]], dtype=np.uint32)
    li = np.array([[0, 1, 2, 3]], dtype=np.int32)
    got = U.ref_select(vals, li, [4], [0], [4], 4, 0, 0, 4)
    # -0 is written as +0; a NaN keeps its sign and payload, a signalling one is quieted
    assert got["out_f32"].view(np.uint32).tolist() == [0x00000000, 0xFFC12345, 0x7FC00001, 0xBF800000]
    assert got["restore"][0].size == 0


def test_branch_model_on_a_hand_counted_record():
    vals = np.array([[0x40000000, 0x3F800600, 0xBF800601, 0x3F800E00, 0x3F000000, U.PAD_BITS]], dtype=np.uint32)
    li = np.array([[5, 4, 3, 2, 1, -1]], dtype=np.int32)
    m = U.branch_model(vals, li, [0], 3)
    assert (m["n"], m["valid"], m["c1"], m["c1_count"], m["need"]) == (6, 5, 0x3F8, 3, 2)
    assert (m["b2"], m["need2"], m["n2"], m["path"]) == (3, 1, 2, "pairwise")
    assert (m["nblk"], m["grid"], m["rounds"], m["shared_copy"]) == (1, 1, 1, False)
    assert m["block_counts"].tolist() == [3]
    m = U.branch_model(vals, li, [0], 1)          # the cut in the bin above: nothing needed below
    assert (m["c1"], m["need"], m["b2"], m["need2"], m["n2"]) == (0x400, 1, 0, 1, 1)
    m = U.branch_model(vals, li, [0], 4)          # need = the whole of C1: the cut sub-bin is its lowest
    assert (m["c1"], m["need"], m["c1_count"], m["b2"], m["need2"], m["n2"]) == (0x3F8, 3, 3, 3, 2, 2)
    m = U.branch_model(vals, li, [0], 6)          # more than the valid entries
    assert (m["c1"], m["need"], m["b2"], m["need2"], m["n2"]) == (-1, 0, U.BINS, 0, 0)


def test_branch_model_blocks_grid_and_radix_passes():
    # 4097 slots: C1 entries at slots 0, 4095 (block 0) and 4096 (block 1)
    vals = np.full((1, 4097), U.BELOW_BITS, dtype=np.uint32)
    vals[0, [0, 4095, 4096]] = U.C1_BITS
    li = np.arange(4097, dtype=np.int32)[None, :]
    m = U.branch_model(vals, li, [0], 2)
    assert m["block_counts"].tolist() == [2, 1] and (m["nblk"], m["grid"], m["rounds"]) == (2, 2, 1)
    assert (m["need"], m["need2"], m["n2"], m["path"]) == (2, 2, 3, "pairwise")
    # 1025 identical entries, global index = slot: the index digits are bits 30..20 (all ones), 19..9
    # (2047 for indices 0..511, 2046 for 512..1023, 2045 for 1024) and 8..0
    vals = np.full((1, 1025), U.C1_BITS, dtype=np.uint32)
    li = np.arange(1025, dtype=np.int32)[None, :]
    for k, passes in ((1025, 1), (512, 5), (1024, 5), (1, 6), (513, 6)):
        m = U.branch_model(vals, li, [0], k)
        assert (m["n2"], m["need2"], m["path"], m["radix_passes"]) == (1025, k, "radix", passes), k
        assert m["index_digits"] == (passes >= 4)
    # low bits i % 512 over 1026 entries: the two entries of low = 511 are cut off by the key alone
    vals = (np.uint32(U.C1_BITS) | (np.arange(1026, dtype=np.uint32) % np.uint32(512)))[None, :]
    li = np.arange(1026, dtype=np.int32)[None, :]
    m = U.branch_model(vals, li, [0], 2)
    assert (m["path"], m["radix_passes"], m["index_digits"]) == ("radix", 3, False)
    m = U.branch_model(vals, li, [0], 1)          # indices 511 and 1023 differ in bit 9: the fifth pass
    assert (m["path"], m["radix_passes"], m["index_digits"]) == ("radix", 5, True)
    # the grid stops at 512 workgroups: 513 blocks are two rounds for workgroup 0
    m = U.branch_model(np.zeros((513, 4096), dtype=np.uint32), np.zeros((513, 4096), dtype=np.int32), [0] * 513, 1)
    assert (m["nblk"], m["grid"], m["rounds"], m["shared_copy"]) == (513, 512, 2, True)


def test_deal_orders_differ_and_indices_are_unique():
    vals, li, sizes = U.deal(np.arange(10, dtype=np.uint32), 3, 5, [4, 2, 4])
    assert sizes == [17, 11, 17]
    assert (li[0, :4] == [9 + 2, 6 + 2, 3 + 2, 2]).all() and (li[0, 4:] == -1).all()
    assert (li[1, :2] == [3 + 1, 1]).all() and (vals[1, 2:] == U.PAD_BITS).all()
    # entries 0, 1, 2 on ranks 0, 1, 2; 6, 7 skip the full rank 1; every third negated
    assert vals[:, 0].tolist() == [0, 1 | 0x80000000, 2]
    assert vals[0].tolist()[:4] == [0, 3, 6, 8] and vals[2].tolist()[:4] == [2, 5, 7 | 0x80000000, 9]


@pytest.mark.parametrize("name", list(U.CASES))
def test_every_gpu_case_reaches_its_branch(name):
    vals, li, sizes, k, expect = U.build_case(name)
    assert vals.dtype == np.uint32 and li.dtype == np.int32 and vals.shape == li.shape
    assert ((li >= 0) | (vals == U.PAD_BITS)).all()
    assert all(int(li[w].max()) < sizes[w] for w in range(len(sizes)))
    valid = int((li >= 0).sum())
    if k is None:
        k = valid // 2
    U.check_model(name, vals, li, sizes, k, expect)
    if "status" in expect:
        got = U.ref_select(vals, li, sizes, U.bases_of(sizes), sizes, k, 0, 0, sum(sizes))
        assert got["status"] == expect["status"]


def test_cut_population_ties_sit_on_different_ranks():
    """beyond 512 entries the cut sub-bin repeats keys: the repeats must be spread over ranks, and
    the cut must fall inside a run of equal keys for some need2 the GPU tests use"""
    for T in (1023, 1024, 1025, 3000):
        vals, li, sizes, k = U.cut_population(T, T - 1)
        key = vals & np.uint32(0x7FFFFFFF)
        in3 = (li >= 0) & ((key >> np.uint32(9)) == np.uint32((U.C1_BITS >> 9) | 3))
        assert int(in3.sum()) == T
        holders, lows = np.nonzero(in3)[0], key[in3] & np.uint32(511)
        repeated = min(T - 512, 512)
        spread = sum(np.unique(holders[lows == low]).size > 1 for low in range(repeated))
        assert 2 * spread > repeated, T
        got = U.ref_select(vals, li, sizes, U.bases_of(sizes), sizes, k, 0, 0, 0)
        cutkeys_sel = set(key[in3 & got["sel"]].tolist())
        cutkeys_rej = set(key[in3 & ~got["sel"]].tolist())
        assert cutkeys_sel & cutkeys_rej, T          # one key on both sides: decided by the global index
        signs = vals[in3] >> np.uint32(31)
        assert 0 < int(signs.sum()) < T
