"""grace_sparse_aggregate_padded_bf16 (records.hip) and grace_randomk_aggregate_bf16 (sparse.hip) on
hand-built buffers, no compressor: bit for bit a numpy restatement of the rank-ordered sum
((0 + d0) + d1) + ..., the division and one rounding (tests/sparse_bf16_util.padded_ref, want_bits).
The padded layout is the threshold counts exchange's: rank w's block of 2 cap words is
[vals f32[cap] | idx i32[cap]], the counts sit in a device int32[W] array, indices ascend within a rank."""
import numpy as np
import pytest
import torch

from grace_amd import ops
from tests.sparse_bf16_util import bits16, padded_ref, want_bits

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = np.float32
CHUNK = 8192      # records.hip kRChunk


def _build(n, W, seed):
    """counts with 0 and cap among them, ranks that share indices, indices on chunk borders, one index out
    of range (ascending order kept: it is the last entry of its rank) and garbage past every count."""
    rng = np.random.default_rng(seed)
    cap = max(1, min(n, 700))
    counts = rng.integers(0, cap + 1, W)
    counts[0] = cap
    if W > 1:
        counts[1] = 0
    if W > 2:
        counts[2] = cap
    shared = np.unique(rng.integers(0, n, max(1, cap // 4)))
    borders = np.array([b for b in (0, CHUNK - 1, CHUNK, 2 * CHUNK - 1, 2 * CHUNK, n - 1) if 0 <= b < n])
    vals = rng.standard_normal((W, cap)).astype(F32)
    idx = np.empty((W, cap), dtype=np.int32)
    for w in range(W):
        c = int(counts[w])
        pool = np.unique(np.concatenate([shared, borders, rng.integers(0, n, c)]))
        pick = np.sort(rng.choice(pool, min(c, pool.size), replace=False)) if c else np.empty(0, dtype=np.int64)
        if w == 2 and n > 1000:     # 300 entries of chunk 0: more than a block-width of one rank in one chunk
            pick = np.unique(np.concatenate([np.arange(300), pick[pick >= 300][:c - 300]]))
        counts[w] = c = pick.size
        idx[w, :c] = pick
        idx[w, c:] = 2 ** 31 - 1 - np.arange(cap - c)   # garbage past the count: huge indices, never entries
        vals[w, c:] = F32(1e30)
    if W > 0 and counts[0] >= 2:
        idx[0, counts[0] - 1] = n                       # one index out of range: skipped
    specials = [np.inf, -np.inf, np.nan, -0.0, F32(3e-39)]
    for j, v in enumerate(specials):
        w = j % W
        if counts[w] > j:
            vals[w, j] = v
    return cap, counts.astype(np.int32), vals, idx


@pytest.mark.parametrize("W", [1, 2, 3, 64, 65])       # 64 | 65: the two sides of the SMALLW split
@pytest.mark.parametrize("n", [1, 8191, 8192, 8193, 50000])
def test_padded_decode_vs_numpy(n, W):
    cap, counts, vals, idx = _build(n, W, 1000 * W + n)
    assert counts.max() == cap or n == 1
    assert (counts == 0).any() or W == 1
    buf = np.empty((W, 2 * cap), dtype=F32)
    buf[:, :cap] = vals
    buf[:, cap:] = idx.view(F32)
    dbuf = torch.from_numpy(buf.ravel()).to(DEV)
    dcnt = torch.from_numpy(counts).to(DEV)
    for divisor in (W, 1):
        out = ops.sparse_aggregate_padded(dbuf, cap, dcnt, W, n, divisor)
        assert out.dtype == torch.bfloat16 and out.shape == (n,)
        assert np.array_equal(bits16(out), want_bits(padded_ref(vals, idx, counts, cap, n, divisor))), (n, W, divisor)


def test_padded_decode_counts_outside_0_cap_are_clamped():
    """A count above cap reads cap entries, a negative one none; nothing past the block is touched."""
    n, W, cap = 8193, 3, 5
    vals = np.arange(1, W * cap + 1, dtype=F32).reshape(W, cap)
    idx = np.array([[0, 1, 8190, 8191, 8192]] * W, dtype=np.int32)
    counts = np.array([cap + 1000, -7, 3], dtype=np.int32)
    buf = np.concatenate([vals, idx.view(F32)], axis=1).ravel()
    out = ops.sparse_aggregate_padded(torch.from_numpy(buf).to(DEV), cap, torch.from_numpy(counts).to(DEV), W, n, 2)
    assert np.array_equal(bits16(out), want_bits(padded_ref(vals, idx, counts, cap, n, 2)))


def test_padded_decode_refuses_what_is_outside_its_limits():
    buf = torch.zeros(2 * 2 * 8, device=DEV)
    cnt = torch.zeros(2, dtype=torch.int32, device=DEV)
    for cap, world, n in ((8, 2, 7), (0, 2, 100), (8, 0, 100), (8, 1025, 100), (8, 2, 2 ** 31)):
        with pytest.raises(ValueError):
            ops.sparse_aggregate_padded(buf, cap, cnt, world, n, 1)
    with pytest.raises(ValueError):
        ops.sparse_aggregate_padded(buf[:-1], 8, cnt, 2, 100, 1)
    with pytest.raises(TypeError):
        ops.sparse_aggregate_padded(buf, 8, cnt.to(torch.int64), 2, 100, 1)
    with pytest.raises(TypeError):
        ops.sparse_aggregate_padded(buf, 8, cnt, 2, 100, 1, out_dtype=torch.float32)


# ------------------------------------------------------------------------------- random-k
@pytest.mark.parametrize("W", [2, 3])
@pytest.mark.parametrize("n", [1, 8193, 50000])
def test_randomk_aggregate_vs_numpy(n, W):
    """vals[w][j] = t_w[idx[j]]: duplicates of an index carry equal values on every rank, as in a step."""
    rng = np.random.default_rng(10 * n + W)
    k = max(1, n // 2)
    idx = rng.integers(0, n, k)
    assert n < 8192 or np.unique(idx).size < k, "the draw was meant to contain duplicates"
    t = rng.standard_normal((W, n)).astype(F32)
    if n > 8:
        t[0, idx[0]], t[1, idx[1]], t[0, idx[2]], t[1, idx[3]] = np.inf, np.nan, -0.0, F32(3e-39)
    vals = np.stack([t[w][idx] for w in range(W)])
    d_idx = torch.from_numpy(idx).to(DEV)
    if n > 8:       # an index outside [0, n) is skipped (it cannot come from a draw)
        bad = idx.copy()
        bad[5], bad[6] = n, -1
        d_idx = torch.from_numpy(bad).to(DEV)
        idx_ok = np.ones(k, dtype=bool)
        idx_ok[5] = idx_ok[6] = False
    else:
        idx_ok = np.ones(k, dtype=bool)
    for divisor in (W, 1):
        acc = np.zeros(n, dtype=F32)
        with np.errstate(invalid="ignore"):
            for w in range(W):
                d = np.zeros(n, dtype=F32)
                d[idx[idx_ok]] = vals[w][idx_ok]
                acc = (acc + d).astype(F32)
            # a position whose only draws were the two replaced ones stays as it is in `acc`: zero unless
            # another duplicate of it was kept, which carries the same value
            want = (acc / F32(divisor)).astype(F32) if divisor != 1 else acc
        out = ops.randomk_aggregate(torch.from_numpy(vals.ravel()).to(DEV), d_idx, W, n, divisor)
        assert out.dtype == torch.bfloat16 and out.shape == (n,)
        assert np.array_equal(bits16(out), want_bits(want)), (n, W, divisor)
    with pytest.raises(TypeError):
        ops.randomk_aggregate(torch.from_numpy(vals.ravel()).to(DEV), d_idx, W, n, 1, out_dtype=torch.float32)
    with pytest.raises(ValueError):
        ops.randomk_aggregate(torch.from_numpy(vals.ravel()[1:]).to(DEV), d_idx, W, n, 1)
