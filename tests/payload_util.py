"""Host side of the world > 1 sparse-decode tests: a sparse reference of the rank-ordered aggregate,
a host builder of the chunk-grouped wire form, and the payload cases shared by the CPU self-test
(tests/test_payload_util.py) and the GPU tests (tests/test_gpu_payload_branches.py)."""
import functools

import numpy as np

F32 = np.float32
CHUNK_LOG = 13
CHUNK = 1 << CHUNK_LOG          # payload.hip kPChunk
POISON = F32(1e30)              # slack past a rank's count: index 0, this value


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def ref_aggregate(payloads, n, divisor):
    """Python's sum of the W dense decodes in rank order, then one division, on the touched elements
    only: (touched indices ascending int64, their f32 values).  Every other element of the dense
    result is +0.0.  payloads = [(vals f32, idx)] in rank order, indices unique within a rank."""
    idx_all = [np.asarray(i, dtype=np.int64).ravel() for _, i in payloads]
    touched = np.unique(np.concatenate(idx_all)) if idx_all else np.zeros(0, np.int64)
    assert touched.size == 0 or (touched[0] >= 0 and touched[-1] < n)
    acc = np.zeros(touched.size, dtype=F32)                 # +0.0
    for (vals, _), idx in zip(payloads, idx_all):
        pos = np.searchsorted(touched, idx)
        assert np.unique(pos).size == pos.size, "indices repeat within a rank"
        acc[pos] = acc[pos] + np.asarray(vals, dtype=F32).ravel()
    if divisor != 1:
        acc = (acc / F32(divisor)).astype(F32)
    return touched, acc


def group_on_host(vals, idx, n, seed=0):
    """The chunk-grouped wire form of one payload as uint32 words: [vals | u16 offsets inside the
    chunk, padded to a word | u32 chunk ends], entries shuffled inside every chunk."""
    idx = np.asarray(idx, dtype=np.int64).ravel()
    vals = np.asarray(vals, dtype=F32).ravel()
    k, nch = idx.size, (n + CHUNK - 1) // CHUNK
    ch = idx >> CHUNK_LOG
    order = np.lexsort((np.random.default_rng(seed).random(k), ch))
    offs = np.zeros(2 * ((k + 1) // 2), dtype=np.uint16)
    offs[:k] = idx[order] & (CHUNK - 1)
    ends = np.cumsum(np.bincount(ch, minlength=nch)).astype(np.uint32)
    return np.concatenate([bits(vals[order]), offs.view(np.uint32), ends])


def draw_values(rng, k):
    """standard_normal * 10**uniform(-3, 3), with a few -0.0 and one quiet NaN."""
    v = (rng.standard_normal(k) * 10.0 ** rng.uniform(-3, 3, k)).astype(F32)
    if k >= 8:
        sp = rng.choice(k, 4, replace=False)
        v[sp[:3]] = F32(-0.0)
        v[sp[3]] = F32(np.nan)
    return v


def distinct(rng, n, k):
    """k distinct integers in [0, n) in random order, without an n-sized array."""
    got = np.zeros(0, np.int64)
    while got.size < k:
        got = np.unique(np.concatenate([got, rng.integers(0, n, 2 * k + 16)]))
    return rng.permutation(got)[:k]


def build_ranks(world, n, table, seed):
    """[(vals f32[k], idx i32[k])] per rank.  table["chunks"][c][w] entries of rank w in chunk c
    (offsets drawn without replacement inside the chunk), and every rank topped up to the common k
    in the chunks of table["fill"]."""
    rng = np.random.default_rng(seed)
    chunks, fill = table["chunks"], tuple(table["fill"])
    room = lambda c: min(CHUNK, n - c * CHUNK)
    totals = [sum(int(chunks[c][w]) for c in chunks) for w in range(world)]
    k = max(totals) + len(fill)
    ranks = []
    for w in range(world):
        per = {c: int(chunks[c][w]) for c in chunks}
        need = k - totals[w]
        for j, c in enumerate(fill):
            assert c not in chunks
            per[c] = need // len(fill) + (1 if j < need % len(fill) else 0)
        parts = []
        for c, cnt in per.items():
            assert 0 <= cnt <= room(c), (c, cnt)
            if cnt:
                parts.append(c * CHUNK + rng.choice(room(c), cnt, replace=False))
        idx = rng.permutation(np.concatenate(parts)).astype(np.int32)
        assert idx.size == k
        ranks.append((draw_values(rng, k), idx))
    return ranks


def gathered_words(ranks, n, seed=0):
    """The W host-grouped payloads back to back (rank-major, stride k + ceil(k/2) + nchunks words)."""
    return np.concatenate([group_on_host(v, i, n, seed + w) for w, (v, i) in enumerate(ranks)])


def order_matters(payloads, n):
    """Whether the aggregate of these payloads changes in at least one bit with the ranks reversed."""
    ta, a = ref_aggregate(payloads, n, 1)
    tb, b = ref_aggregate(payloads[::-1], n, 1)
    assert np.array_equal(ta, tb)
    return bool(np.any(bits(a) != bits(b)))


# ---------------------------------------------------------------- one-pass aggregate (B)
BASE_N = 6 * CHUNK + 5
SORTED_WORLDS = (1, 2, 8, 9, 63, 64, 65, 257, 1024)
_COUNTS = (0, 1, 255, 256, 257, 513, 8192, 2)       # per-rank entries of a chunk, selected by w % 8
SORTED_LARGE = ((3, (1 << 26) + 2 * CHUNK + 5, 5000), (2, 1 << 28, 3000))


@functools.lru_cache(maxsize=2)
def sorted_base_case(world, n=BASE_N):
    """Chunks 0 and 2 hold 0 .. 8192 entries of a rank (below, at and above the kernel's 256-entry
    round, and a full chunk), the last chunk a few, chunks 1, 3 and 4 the fillers."""
    last = (n - 1) >> CHUNK_LOG
    table = {"chunks": {0: [_COUNTS[w % 8] for w in range(world)],
                        2: [_COUNTS[(w + 3) % 8] for w in range(world)],
                        last: [w % 6 for w in range(world)]},
             "fill": (1, 3, 4)}
    return build_ranks(world, n, table, seed=1000 + world)


@functools.lru_cache(maxsize=1)
def sorted_large_case(world, n, k):
    """Half of every rank's indices shared by all ranks, the rest its own; the first and last chunks
    and the chunks on both sides of every 8192-chunk scan round hold entries."""
    rng = np.random.default_rng(world + k)
    nch = (n + CHUNK - 1) // CHUNK
    edge = [0, nch - 1] + [c for m in range(8192, nch, 8192) for c in (m - 1, m)]
    forced = np.array([c * CHUNK + min(7, n - c * CHUNK - 1) for c in edge], dtype=np.int64)
    shared = np.setdiff1d(distinct(rng, n, k // 2), forced)
    ranks = []
    for _ in range(world):
        own = np.setdiff1d(distinct(rng, n, k), np.concatenate([shared, forced]))
        idx = np.concatenate([forced, shared, own])[:k]
        ranks.append((draw_values(rng, k), rng.permutation(idx).astype(np.int32)))
    return ranks


# ---------------------------------------------------------------- scatter / tag aggregate (C)
SCATTER_N = 100003
SCATTER_STRIDE = 1024
SCATTER_COUNTS = ((0, 700, 13), (700, 0, 13), (13, 700, 0), tuple((w * 37) % 300 for w in range(64)))
SCATTER_LARGE = (2, (1 << 28) + CHUNK + 3, 3000)


def _pooled_ranks(rng, counts, n):
    """Every rank draws its indices from one small pool, so the ranks overlap heavily."""
    pool = distinct(rng, n, max(max(counts) * 3 // 2, 8))
    ranks = []
    for c in counts:
        idx = rng.choice(pool, c, replace=False).astype(np.int32)
        ranks.append((draw_values(rng, c), idx))
    return ranks


@functools.lru_cache(maxsize=4)
def scatter_case(counts, n=SCATTER_N, stride=SCATTER_STRIDE):
    """(ranks, vals f32[W, stride], idx i32[W, stride]); the slack past a rank's count is poison."""
    rng = np.random.default_rng(sum((j + 1) * c for j, c in enumerate(counts)))
    ranks = _pooled_ranks(rng, counts, n)
    vals = np.full((len(counts), stride), POISON, dtype=F32)
    idx = np.zeros((len(counts), stride), dtype=np.int32)
    for w, (v, i) in enumerate(ranks):
        vals[w, :v.size] = v
        idx[w, :i.size] = i
    return ranks, vals, idx


# ---------------------------------------------------------------- capped records (D)
CAPPED_N = 50021
CAP = 1000
CAPPED_COUNTS = ((0,), (1,), (999,), (1000,), (1001,), (5000,),
                 (999, 1000, 1001), (1001, 5000, 999),
                 (1, 1000, 5000, 0, 999), (1000, 999, 1, 0, 1000))


@functools.lru_cache(maxsize=4)
def capped_case(counts, cap=CAP, n=CAPPED_N):
    """(live ranks, records i32[W, 4 + 2 cap]) with {count, cap, 0, 0 | vals[cap] | idx[cap]}: only the
    first min(count, cap) entries are live, the rest is poison."""
    rng = np.random.default_rng(7 + sum((j + 3) * c for j, c in enumerate(counts)))
    ranks = _pooled_ranks(rng, tuple(min(c, cap) for c in counts), n)
    recs = np.zeros((len(counts), 4 + 2 * cap), dtype=np.uint32)
    for w, (v, i) in enumerate(ranks):
        recs[w, 0], recs[w, 1] = counts[w], cap
        recs[w, 4:4 + cap] = bits(np.full(cap, POISON, dtype=F32))
        recs[w, 4:4 + v.size] = bits(v)
        recs[w, 4 + cap:4 + cap + i.size] = i.view(np.uint32)
    return ranks, recs.view(np.int32)


def order_cases():
    """(name, payloads, n) of every aggregate case with three ranks or more."""
    for world in SORTED_WORLDS:
        if world >= 3:
            yield f"sorted-w{world}", sorted_base_case(world), BASE_N
    yield "sorted-w9-whole", sorted_base_case(9, 6 * CHUNK), 6 * CHUNK
    for world, n, k in SORTED_LARGE:
        if world >= 3:
            yield f"sorted-large-w{world}", sorted_large_case(world, n, k), n
    for counts in SCATTER_COUNTS:
        yield f"scatter-{len(counts)}-{counts[0]}", scatter_case(counts)[0], SCATTER_N
    for counts in CAPPED_COUNTS:
        if len(counts) >= 3:
            yield f"capped-{counts}", capped_case(counts)[0], CAPPED_N
