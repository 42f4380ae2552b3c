"""The world > 1 sparse decode on every launch branch: grace_sort_payload and
grace_sparse_aggregate_sorted (payload.hip), grace_sparse_aggregate[_into] (topk.hip) and
grace_sparse_aggregate_capped (sparse.hip), bit for bit against tests/payload_util.ref_aggregate.

The aggregate tests take host-grouped payloads (payload_util.group_on_host), so they do not depend on
the grouping kernels; from n = 2^26 on the dense output stays on the device: it is gathered at the
touched indices, and every other element must have zero bits."""
import os
import tempfile

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from grace_amd import _lib, ops
from tests import payload_util as U

pytestmark = pytest.mark.gpu
DEV = "cuda"
CH = U.CHUNK


def _dev(words):
    """uint32 / int32 / float32 host words -> a float32 device tensor with the same bits."""
    return torch.from_numpy(np.ascontiguousarray(words).view(np.float32)).to(DEV)


def _check_dense(out, ranks, n, divisor, what):
    touched, ref = U.ref_aggregate(ranks, n, divisor)
    exp = np.zeros(n, dtype=np.uint32)
    exp[touched] = U.bits(ref)
    got = out.cpu().numpy().view(np.uint32)
    assert got.size == n and np.array_equal(got, exp), (what, np.flatnonzero(got != exp)[:8])


def _check_on_device(out, ranks, n, divisor, what):
    touched, ref = U.ref_aggregate(ranks, n, divisor)
    assert out.numel() == n
    got = out[torch.from_numpy(touched).to(DEV)].cpu().numpy().view(np.uint32)
    assert np.array_equal(got, U.bits(ref)), (what, touched[np.flatnonzero(got != U.bits(ref))[:8]])
    assert int(torch.count_nonzero(out.view(torch.int32))) == int(np.count_nonzero(U.bits(ref))), what


def _divisors(world):
    return tuple(dict.fromkeys((world, 1, 3)))


# ------------------------------------------------------------------------------- A. grouping
def _check_grouping(vals, idx, n):
    k, nch, ow = idx.size, (n + CH - 1) // CH, (idx.size + 1) // 2
    buf = _dev(np.concatenate([U.bits(vals), idx.astype(np.int32).view(np.uint32)]))
    out = ops.sort_payload(buf, k, n).cpu().numpy().view(np.uint32)
    assert out.size == ops.sorted_payload_len(k, n) == k + ow + nch
    offs = out[k:k + ow].view(np.uint16)[:k].astype(np.int64)
    ends = out[k + ow:].astype(np.int64)
    assert np.all(np.diff(ends) >= 0), (n, k)
    assert ends[-1] == k, (n, k)
    per = np.bincount(idx.astype(np.int64) >> 13, minlength=nch)
    assert np.array_equal(np.diff(ends, prepend=0), per), (n, k, np.flatnonzero(np.diff(ends, prepend=0) != per)[:8])
    assert np.all(offs < CH), (n, k)
    back = np.searchsorted(ends, np.arange(k), side="right") * CH + offs
    o1, o2 = np.argsort(back, kind="stable"), np.argsort(idx, kind="stable")
    assert np.array_equal(back[o1], idx[o2].astype(np.int64)), (n, k)
    assert np.array_equal(out[:k][o1], U.bits(vals)[o2]), (n, k)


def _payload(idx, seed):
    idx = np.asarray(idx, dtype=np.int64)
    assert np.unique(idx).size == idx.size
    rng = np.random.default_rng(seed)
    return U.draw_values(rng, idx.size), rng.permutation(idx).astype(np.int32)


@pytest.mark.parametrize("n,idx", [(100, [57]), (8191, np.arange(8191)), (8193, [8191, 8192])],
                         ids=["n100-k1", "n8191-k8191", "n8193-k2"])
def test_group_one_or_two_chunks(n, idx):
    """k = 1; a full single chunk, whose two workgroups share one cursor; the two sides of the first
    chunk edge."""
    _check_grouping(*_payload(idx, n), n)


@pytest.mark.parametrize("k", [1023, 1025, 4096, 4097])
def test_group_workgroup_edges(k):
    """One thread round and one workgroup (4096 entries), less and more; odd k pads the u16 offsets."""
    n = 5 * CH + 7
    _check_grouping(*_payload(U.distinct(np.random.default_rng(k), n, k), k), n)


def test_group_cursor_contention():
    """20000 entries in three chunks: five workgroups reserve ranges in the same three cursors, and
    every chunk holds more entries than one workgroup brings."""
    n, k, chunks = 1 << 20, 20000, np.array([0, 63, 127])
    pos = U.distinct(np.random.default_rng(20), 3 * CH, k)
    idx = chunks[pos // CH] * CH + pos % CH
    assert np.bincount(idx >> 13, minlength=128)[chunks].min() > 4096
    _check_grouping(*_payload(idx, 21), n)


def _scan_round_payload(nch, n, k=3000):
    """Entries forced into the first and last chunk and into the chunks on both sides of every
    multiple of 8192 chunks (one scan round of the counts), at the chunk's first and last element."""
    edge = sorted({0, nch - 1} | {c for m in range(8192, nch + 1, 8192) for c in (m - 1, m) if c < nch})
    forced = np.unique(np.array([c * CH + o for c in edge for o in (0, min(CH, n - c * CH) - 1)], dtype=np.int64))
    rest = np.setdiff1d(U.distinct(np.random.default_rng(nch), n, k), forced)[:k - forced.size]
    return _payload(np.concatenate([forced, rest]), nch)


@pytest.mark.parametrize("nch", [8191, 8192, 8193, 16385])
def test_group_scan_rounds(nch):
    """The exclusive scan of the chunk counts covers 8192 chunks per round: one round less one chunk,
    one round exactly, a second round of one chunk, a third round of one chunk."""
    n = nch * CH - 3
    _check_grouping(*_scan_round_payload(nch, n), n)


def test_group_at_the_promised_limit_leaves_the_workspace_zeroed():
    """n = 2^28 = ops.SORT_PAYLOAD_MAX_N: 32768 chunks, four scan rounds, 128 KiB of dynamic LDS per
    workgroup.  A small grouping on the same workspace afterwards finds counts and cursors zeroed."""
    n = 1 << 28
    assert n == ops.SORT_PAYLOAD_MAX_N
    _check_grouping(*_scan_round_payload(n // CH, n), n)
    m = 100003
    _check_grouping(*_payload(U.distinct(np.random.default_rng(5), m, 1000), 6), m)


# ------------------------------------------------------------------------------- B. one-pass aggregate
@pytest.mark.parametrize("world", U.SORTED_WORLDS)
def test_sorted_aggregate_every_rank_count_and_world(world):
    """Per-rank entries of a chunk below, at and above the 256-entry round up to a full chunk, an
    empty chunk, a 5-element last chunk; worlds inside one rank batch (1, 2, 8), with a clamped
    second batch (9, 63), at the register-bounds limit (64) and on the LDS bounds table whose fill
    takes one (65), two (257) and four (1024) strides of the 256 threads."""
    n = U.BASE_N
    ranks = U.sorted_base_case(world)
    k = ranks[0][1].size
    g = _dev(U.gathered_words(ranks, n))
    assert g.numel() == world * ops.sorted_payload_len(k, n)
    for divisor in _divisors(world):
        _check_dense(ops.sparse_aggregate_sorted(g, k, world, n, divisor), ranks, n, divisor, (world, divisor))


def _sorted_call(g, k, stride, world, divisor, out, n):
    ow = (k + 1) // 2
    _lib.call("grace_sparse_aggregate_sorted", g.data_ptr(), g[k:].data_ptr(), g[k + ow:].data_ptr(), stride,
              world, float(divisor), out.data_ptr(), n, ops._stream())


@pytest.mark.parametrize("shift", [0, 1])
def test_sorted_aggregate_whole_last_chunk_and_unaligned_out(shift):
    """n = 6 * 8192: the last chunk is whole and takes the vector store; with `out` one float past a
    16-byte boundary every chunk takes the scalar store instead.  The floats around `out` stay."""
    world, n = 9, 6 * CH
    ranks = U.sorted_base_case(world, n)
    k = ranks[0][1].size
    g = _dev(U.gathered_words(ranks, n))
    for divisor in _divisors(world):
        big = torch.full((n + 8,), 7.5, dtype=torch.float32, device=DEV)
        assert big.data_ptr() % 16 == 0
        out = big[4 * (1 - shift) + 5 * shift:][:n]                      # 16 B aligned, or 4 B past it
        assert out.data_ptr() % 16 == 4 * shift
        _sorted_call(g, k, ops.sorted_payload_len(k, n), world, divisor, out, n)
        _check_dense(out, ranks, n, divisor, (shift, divisor))
        rest = torch.cat([big[:4 + shift], big[4 + shift + n:]]).cpu().numpy()
        assert np.all(rest == np.float32(7.5)), (shift, divisor)
    if shift:   # the same on a partial last chunk
        ranks = U.sorted_base_case(world)
        n, k = U.BASE_N, ranks[0][1].size
        g = _dev(U.gathered_words(ranks, n))
        big = torch.full((n + 8,), 7.5, dtype=torch.float32, device=DEV)
        _sorted_call(g, k, ops.sorted_payload_len(k, n), world, 3, big[1:1 + n], n)
        _check_dense(big[1:1 + n], ranks, n, 3, "partial")
        assert np.all(torch.cat([big[:1], big[1 + n:]]).cpu().numpy() == np.float32(7.5))


@pytest.mark.parametrize("world,n,k", U.SORTED_LARGE, ids=["w3-2p26", "w2-2p28"])
def test_sorted_aggregate_large(world, n, k):
    """More than 8192 output chunks, up to the 32768 the entry accepts."""
    ranks = U.sorted_large_case(world, n, k)
    g = _dev(U.gathered_words(ranks, n))
    for divisor in (world, 1):
        out = ops.sparse_aggregate_sorted(g, k, world, n, divisor)
        _check_on_device(out, ranks, n, divisor, (world, divisor))
        del out


# ------------------------------------------------------------------------------- C. scatter / tag aggregate
@pytest.mark.parametrize("counts", U.SCATTER_COUNTS, ids=["0-700-13", "700-0-13", "13-700-0", "w64"])
@pytest.mark.parametrize("prefilled", [False, True], ids=["alloc", "into"])
def test_scatter_aggregate_unequal_counts(counts, prefilled):
    """Counts that differ between ranks, an empty first, middle or last rank, world 64, poisoned slack
    between a rank's count and the stride; the allocating entry and the prefilled-output entry."""
    ranks, vals, idx = U.scatter_case(counts)
    world, n = len(counts), U.SCATTER_N
    dv, di = _dev(vals).view(-1), _dev(idx).view(torch.int32).view(-1)
    for divisor in (world, 1):
        out = torch.zeros(n, dtype=torch.float32, device=DEV) if prefilled else None
        got = ops.sparse_aggregate(dv, di, U.SCATTER_STRIDE, counts, world, n, divisor, out=out)
        assert out is None or got is out
        _check_dense(got, ranks, n, divisor, (counts[:3], prefilled, divisor))


def test_scatter_aggregate_refuses_world_65_and_goes_on():
    world, n = 65, 4099
    dv = torch.ones(world * 8, dtype=torch.float32, device=DEV)
    di = torch.arange(world * 8, dtype=torch.int32, device=DEV)
    for out in (None, torch.zeros(n, dtype=torch.float32, device=DEV)):
        with pytest.raises(_lib.GraceNativeError, match="1 <= world <= 64"):
            ops.sparse_aggregate(dv, di, 8, [8] * world, world, n, world, out=out)
        if out is not None:
            assert int(torch.count_nonzero(out)) == 0
        torch.cuda.synchronize()
        ranks, vals, idx = U.scatter_case(U.SCATTER_COUNTS[0])
        got = ops.sparse_aggregate(_dev(vals).view(-1), _dev(idx).view(torch.int32).view(-1), U.SCATTER_STRIDE,
                                   U.SCATTER_COUNTS[0], 3, U.SCATTER_N, 3)
        _check_dense(got, ranks, U.SCATTER_N, 3, "after the refusal")


def test_scatter_aggregate_above_the_grouping_limit():
    """n = 2^28 + 8192 + 3, the packed [vals | idx] payloads of two ranks: the decode that
    compressor/topk.py takes above ops.SORT_PAYLOAD_MAX_N."""
    world, n, k = U.SCATTER_LARGE
    assert n > ops.SORT_PAYLOAD_MAX_N
    ranks = U.sorted_large_case(world, n, k)
    g = _dev(np.concatenate([np.concatenate([U.bits(v), i.view(np.uint32)]) for v, i in ranks]))
    for divisor in (world, 1):
        out = ops.sparse_aggregate(g, g[k:].view(torch.int32), 2 * k, [k] * world, world, n, divisor)
        _check_on_device(out, ranks, n, divisor, divisor)
        del out


# ------------------------------------------------------------------------------- D. capped records
@pytest.mark.parametrize("counts", U.CAPPED_COUNTS, ids=lambda c: "-".join(map(str, c)))
def test_capped_aggregate_counts_around_the_capacity(counts):
    """Header counts 0, 1, cap - 1, cap, cap + 1 and 5 cap: only min(count, cap) entries are read (the
    rest of the record is poison), and stat = {max count, max count > cap}."""
    ranks, recs = U.capped_case(counts)
    world, n = len(counts), U.CAPPED_N
    drecs = torch.from_numpy(recs).to(DEV).view(-1)
    for divisor in (world, 1):
        stat = torch.full((2,), -1, dtype=torch.int32, device=DEV)
        out = ops.sparse_aggregate_capped(drecs, U.CAP, world, n, divisor, stat)
        assert stat.cpu().tolist() == [max(counts), int(max(counts) > U.CAP)], (counts, divisor)
        _check_dense(out, ranks, n, divisor, (counts, divisor))


# ------------------------------------------------------------------------------- E. the compressor's switch
def _switch_worker(rank, path, outdir):
    dist.init_process_group("gloo", init_method=f"file://{path}", rank=rank, world_size=2)
    torch.cuda.set_device(0)
    from grace_amd.dist.communicator.allgather import Allgather
    from grace_amd.dist.compressor.topk import TopKCompressor
    from grace_amd.dist.memory.residual import ResidualMemory
    calls = {"scatter": 0, "sorted": 0}
    scatter, grouped = ops.sparse_aggregate, ops.sparse_aggregate_sorted

    def count(name, f):
        def g(*a, **kw):
            calls[name] += 1
            return f(*a, **kw)
        return g
    ops.sparse_aggregate, ops.sparse_aggregate_sorted = count("scatter", scatter), count("sorted", grouped)
    res = {}
    for tag, limit in (("grouped", None), ("lowered", 1 << 16)):
        if limit is not None:
            ops.SORT_PAYLOAD_MAX_N = limit
        comm = Allgather(TopKCompressor(0.01), ResidualMemory(), 2)
        for s in range(2):
            g = np.random.default_rng(500 * rank + s).standard_normal(100003).astype(np.float32)
            res[f"g{s}"] = g
            res[f"{tag}_out{s}"] = comm.step(torch.from_numpy(g).cuda(), "w").cpu().numpy()
            res[f"{tag}_res{s}"] = comm.memory.residuals["w"].cpu().numpy()
        res[f"{tag}_calls"] = np.array([calls["scatter"], calls["sorted"]])
    np.savez(os.path.join(outdir, f"r{rank}.npz"), **res)
    dist.destroy_process_group()


def test_topk_world2_switches_to_the_scatter_decode_above_the_limit():
    """Allgather(TopK, ResidualMemory) at world 2, n = 100003, two steps: with
    ops.SORT_PAYLOAD_MAX_N lowered to 2^16 the step decodes with the rank-ordered scatter instead of
    the grouped payloads, and both equal the oracle (and so each other) bit for bit."""
    from oracle import grace_oracle as O
    with tempfile.TemporaryDirectory() as tmp:
        mp.spawn(_switch_worker, args=(os.path.join(tmp, "rdv"), tmp), nprocs=2, join=True)
        zs = [dict(np.load(os.path.join(tmp, f"r{r}.npz"))) for r in range(2)]
    for z in zs:
        assert z["grouped_calls"].tolist() == [0, 2] and z["lowered_calls"].tolist() == [2, 2]
    res = [None, None]
    for s in range(2):
        decs = []
        for r in range(2):
            t, vals, idx, res[r], _ = O.topk_residual_step(zs[r][f"g{s}"], res[r], 0.01)
            decs.append(O.sparse_decode(vals, idx, t.size))
        exp = (O.python_sum(decs) / np.float32(2)).astype(np.float32)
        for r in range(2):
            for tag in ("grouped", "lowered"):
                assert np.array_equal(U.bits(zs[r][f"{tag}_out{s}"]), U.bits(exp)), (tag, s, r)
                assert np.array_equal(U.bits(zs[r][f"{tag}_res{s}"]), U.bits(res[r])), (tag, s, r)
            assert np.array_equal(U.bits(zs[r][f"lowered_out{s}"]), U.bits(zs[r][f"grouped_out{s}"])), (s, r)
            assert np.array_equal(U.bits(zs[r][f"lowered_res{s}"]), U.bits(zs[r][f"grouped_res{s}"])), (s, r)
