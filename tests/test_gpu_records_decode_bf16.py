"""grace_sparse_aggregate_records_bf16 (ops.sparse_aggregate_capped(..., out_dtype=bfloat16)) on
hand-built capacity-bounded records, with no DGC in front of it.

The reference is numpy: the rank-ordered sum ((0 + d0) + d1) + ... in f32, one division, then one
rounding to bf16 (tests/shard_select_util.round_cpu).  The result must also equal the f32 decode of
the same records rounded, and ``stat`` must be what the f32 decode sets.  The kernel's chunk is 8192
output elements and its workgroup 256 threads: the sizes sit on and around a chunk, and one case puts
more entries of a single rank into one chunk than a workgroup has threads."""
import numpy as np
import pytest
import torch

from grace_amd import ops
from tests.shard_select_util import round_cpu

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = np.float32
CHUNK, BLOCK, HDR = 8192, 256, 4
SIZES = [1, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 1, 50000]


def build(entries, cap, header_counts=None, garbage_seed=0):
    """entries[w] = (idx ascending int array, vals f32 array) -> the W records as one int32 tensor.
    The unused tail of vals / idx holds garbage (NaN patterns and indices inside n); header_counts
    overrides the count words (a count above cap: only the first cap entries are valid)."""
    W = len(entries)
    stride = HDR + 2 * cap
    rng = np.random.default_rng(garbage_seed)
    recs = np.zeros((W, stride), dtype=np.uint32)
    for w, (idx, vals) in enumerate(entries):
        c = len(idx)
        assert c <= cap and np.all(np.diff(idx) > 0)
        recs[w, 0] = c if header_counts is None else header_counts[w]
        recs[w, 1] = cap
        recs[w, HDR:HDR + cap] = rng.integers(0x7FC00000, 0x7FFFFFFF, cap, dtype=np.uint32)      # NaNs
        recs[w, HDR + cap:] = rng.integers(0, 4, cap, dtype=np.uint32)                           # live indices
        recs[w, HDR:HDR + c] = np.asarray(vals, dtype=F32).view(np.uint32)
        recs[w, HDR + cap:HDR + cap + c] = np.asarray(idx, dtype=np.int32).view(np.uint32)
    return torch.from_numpy(recs.view(np.int32).reshape(-1)).to(DEV)


def reference(entries, n, divisor):
    acc = np.zeros(n, dtype=F32)
    with np.errstate(invalid="ignore", over="ignore"):
        for idx, vals in entries:
            d = np.zeros(n, dtype=F32)
            d[np.asarray(idx, dtype=np.int64)] = np.asarray(vals, dtype=F32)
            acc = (acc + d).astype(F32)              # ((0 + d0) + d1) + ...: untouched elements stay +0
        # the f32 decode divides the touched elements only; 0 / divisor is +0 either way
        out = (acc / F32(divisor)).astype(F32) if divisor != 1 else acc
    return out


def want_bits(out32):
    return round_cpu(torch.from_numpy(out32)).numpy().astype(np.uint16).view(np.int16)


def decode(recs, cap, W, n, divisor, offset=0):
    stat = torch.full((2,), -1, dtype=torch.int32, device=DEV)
    if offset == 0:
        out = ops.sparse_aggregate_capped(recs, cap, W, n, divisor, stat, out_dtype=torch.bfloat16)
    else:   # out one element into a 16-byte aligned buffer: the scalar epilogue
        from grace_amd import _lib
        buf = torch.full((n + 8,), 7.0, dtype=torch.bfloat16, device=DEV)
        out = buf[offset:offset + n]
        nbytes = _lib.query("grace_sparse_aggregate_records_bf16_workspace_bytes", W, n)
        ws = ops.workspace("records_bf16", nbytes, recs.device)
        _lib.call("grace_sparse_aggregate_records_bf16", recs.data_ptr(), HDR + 2 * cap, cap, W, float(divisor),
                  out.data_ptr(), n, stat.data_ptr(), ws.data_ptr(), nbytes, ops._stream())
        assert torch.all(buf[:offset].float() == 7.0) and torch.all(buf[offset + n:].float() == 7.0)
    assert out.dtype == torch.bfloat16 and out.numel() == n
    return out.view(torch.int16).cpu().numpy(), stat.cpu().numpy()


def check(entries, cap, n, divisor, header_counts=None, offset=0, what=None):
    W = len(entries)
    recs = build(entries, cap, header_counts)
    got, stat = decode(recs, cap, W, n, divisor, offset)
    want = want_bits(reference(entries, n, divisor))
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (what, bad[:5], got[bad[:5]], want[bad[:5]])
    stat32 = torch.full((2,), -1, dtype=torch.int32, device=DEV)
    out32 = ops.sparse_aggregate_capped(recs, cap, W, n, divisor, stat32)
    assert np.array_equal(got, want_bits(out32.cpu().numpy())), what
    assert np.array_equal(stat, stat32.cpu().numpy()), (what, stat, stat32)
    mx = max(header_counts) if header_counts is not None else max(len(i) for i, _ in entries)
    assert stat.tolist() == [mx, int(mx > cap)], (what, stat)


def random_entries(W, n, counts, seed):
    rng = np.random.default_rng(seed)
    out = []
    for w in range(W):
        idx = np.sort(rng.choice(n, counts[w], replace=False)).astype(np.int32)
        vals = rng.standard_normal(counts[w]).astype(F32)
        out.append((idx, vals))
    return out


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("W", [1, 2, 3, 8])
def test_world_divisor_sizes_counts(W, n):
    """Counts 0, exactly cap and in between, ranks overlapping at random; the first and the last index
    of every chunk and of n are hit; divisor 1 and W."""
    cap = max(1, min(n, 300))
    counts = [(0, cap, cap // 2, 1)[w % 4] if n > 1 else w % 2 for w in range(W)]
    counts = [min(c, n) for c in counts]
    entries = random_entries(W, n, counts, 13 * n + W)
    edges = sorted({0, n - 1} | {c for c in range(0, n, CHUNK)} | {c - 1 for c in range(CHUNK, n + 1, CHUNK)})
    w_edge = W - 1                                       # the last rank also holds every chunk edge
    assert len(edges) <= cap
    rest = [i for i in entries[w_edge][0].tolist() if i not in edges][:cap - len(edges)]
    idx = np.array(sorted(edges + rest), dtype=np.int32)
    entries[w_edge] = (idx, np.random.default_rng(n).standard_normal(idx.size).astype(F32))
    for divisor in (1, W):
        check(entries, cap, n, divisor, what=(W, n, divisor))


@pytest.mark.parametrize("n", [CHUNK + 1, 50000])
def test_header_count_above_cap(n):
    """The header says more than cap were selected: only the first cap entries travelled and count;
    stat reports the overflow as the f32 decode does."""
    W, cap = 3, 200
    entries = random_entries(W, n, [cap, 17, cap], 5)
    check(entries, cap, n, W, header_counts=[cap + 100, 17, cap], what="overflow")
    check(entries, cap, n, 1, header_counts=[cap, 17, 4 * cap], what="overflow in the last rank")


def test_one_rank_fills_a_chunk_past_the_block_width():
    """Rank 1 has 3 * 256 + 5 entries in chunk 2 (four rounds of the workgroup) and nothing else; rank
    0 and rank 2 hit some of the same elements, so rank 1's rounds must all land before rank 2's;
    chunks 0, 1, 3, 4 and 5 are empty."""
    n = 6 * CHUNK + 3
    m = 3 * BLOCK + 5
    rng = np.random.default_rng(3)
    dense = (2 * CHUNK + np.sort(rng.choice(CHUNK, m, replace=False))).astype(np.int32)
    shared = dense[::7]
    big = F32(2.0 ** 25)                                 # (big + 1) - big = 0 but (big - big) + 1 = 1
    entries = [(shared, np.full(shared.size, big, dtype=F32)),
               (dense, np.ones(m, dtype=F32)),
               (shared, np.full(shared.size, -big, dtype=F32))]
    for divisor in (1, 3):
        check(entries, m, n, divisor, what=("dense chunk", divisor))
        check(entries, m, n, divisor, offset=1, what=("dense chunk, out offset", divisor))


def test_summation_order_shows():
    """Every rank hits index 5 (and the first index of chunk 1): 1e8 + 1 - 1e8 is 0 in rank order and
    1 in any order that adds the small term last."""
    n = CHUNK + 10
    idx = np.array([5, CHUNK], dtype=np.int32)
    for vals in ([1e8, 1.0, -1e8], [1.0, 1e8, -1e8], [-1e8, 1e8, 1.0]):
        entries = [(idx, np.full(2, v, dtype=F32)) for v in vals]
        ref = reference(entries, n, 1)
        assert ref[5] == F32(F32(F32(0) + F32(vals[0])) + F32(vals[1])) + F32(vals[2])
        check(entries, 2, n, 1, what=vals)
        check(entries, 2, n, 3, what=vals)
    assert reference([(idx, np.full(2, v, dtype=F32)) for v in (1e8, 1.0, -1e8)], n, 1)[5] == 0
    assert reference([(idx, np.full(2, v, dtype=F32)) for v in (-1e8, 1e8, 1.0)], n, 1)[5] == 1


@pytest.mark.parametrize("offset", [0, 1])
def test_special_values_and_out_alignment(offset):
    """NaN, +-inf and -0 values (a lone -0 decodes to 0 + -0 = +0; inf + -inf across ranks is NaN,
    0x7FC0 in bf16), values that round up into the next bf16 and bf16 subnormals."""
    n = 2 * CHUNK + 77
    idx = np.array([0, 1, 2, 3, 4, 5, 6, CHUNK - 1, CHUNK, n - 1], dtype=np.int32)
    v0 = np.array([np.nan, np.inf, -np.inf, -0.0, np.inf, 1.00390625, 3e-39, -0.0, 65280.5, 3.3895e38], dtype=F32)
    v1 = np.array([1.0, 1.0, 1.0, -0.0, -np.inf, 2.0 ** -9, 1e-40, 1.0, 255.5, 3.3895e38], dtype=F32)
    entries = [(idx, v0), (idx, v1)]
    for divisor in (1, 2):
        check(entries, idx.size, n, divisor, offset=offset, what=("specials", divisor, offset))
    check([(idx, v0)], idx.size, n, 1, offset=offset, what=("specials, one rank", offset))


def test_idle_lanes_do_not_read_the_tail():
    """cap far above the counts: the tails of vals and idx hold NaN patterns and indices 0..3; none
    of it may reach the result (elements 0..3 stay +0 unless a valid entry hits them)."""
    n, cap = 3 * CHUNK, 2048
    entries = random_entries(4, n, [3, 0, 700, 1], 21)
    entries = [(np.where(i < 4, i + 4, i).astype(np.int32), v) for i, v in entries]
    entries = [(np.unique(i), v[:np.unique(i).size]) for i, v in entries]
    check(entries, cap, n, 4, what="tails")
    recs = build(entries, cap)
    got, _ = decode(recs, cap, 4, n, 4)
    assert not got[:4].any()
