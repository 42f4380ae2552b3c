"""grace_shard_select on hand-built records (test infrastructure, numpy / torch-CPU only):

  ref_select     the select restated from the contract in include/grace_hip.h: the first
                 min(k, valid) gathered entries by (|t| bits descending, global index ascending);
  branch_model   the kernel's BOOKKEEPING only (csrc/shard.hip: bins, counts, list blocks, which
                 path the last arriver takes, the grid), so a test can assert that a case reaches
                 the branch it is named after before it looks at what the kernel wrote;
  builders       records of bit patterns 0x3F800000 | (s << 9) | low (coarse bin 1016, sub-bin s)
                 with entries above (0x40000000 ..) and below (0x3F000000 ..) that bin, dealt over
                 ranks and slots so that entry order, key order and global-index order all differ;
  CASES          every builder / parameter pair the GPU tests run, with the branch each must reach
                 (tests/test_shard_select_util.py checks them all on the CPU).
"""
import numpy as np
import torch

HDR = 8               # record header words (word 0 = the shard length)
LIST_BLOCK = 4096     # entries per apply round = one block of the C1 list
BINS = 2048           # coarse bins (key >> 20) and sub-bins (key bits 19..9)
GROUPS = 8            # histogram copies (blockIdx % 8)
PAIR_CAP = 1024       # cut entries ranked pairwise; more go through the radix select
MAX_GRID = 512
MAX_WORLD = 1024

C1_BITS = 0x3F800000  # | (s << 9) | low: coarse bin 1016, sub-bin s
ABOVE_BITS = 0x40000000
BELOW_BITS = 0x3F000000
C1_BIN = C1_BITS >> 20
PAD_BITS = 0xFFFFFFFF  # what a padding slot's value holds here: the largest key there is


def round_cpu(out32):
    """The f32 dense result rounded once, on the CPU: the reference of every bf16 output here.
    torch's CPU cast rounds to nearest even; what it makes of a NaN depends on the build (its
    vectorised path gives 0xFFFF), so a NaN position is held to the pattern the kernels define,
    0x7FC0 exactly -- not merely to being a NaN."""
    x = out32.detach().cpu()
    b = x.to(torch.bfloat16).contiguous().view(torch.int16).to(torch.int32) & 0xFFFF
    b[torch.isnan(x)] = 0x7FC0
    return b


# ------------------------------------------------------------------------------- the reference
def ref_select(vals_u32, li, sizes, bases, hdr_m, k, rank, out_base, out_len, sel=None):
    """What grace_shard_select leaves for `rank` (include/grace_hip.h).  Valid entries have
    li >= 0; their order is (bits & 0x7FFFFFFF descending, global index ascending); the first
    min(k, valid) are selected.  `sel`: an earlier result's selection for the same records and k
    (another rank or window of one case: the sort is not repeated)."""
    v = np.ascontiguousarray(vals_u32, dtype=np.uint32)
    li = np.asarray(li, dtype=np.int64)
    world, cap = v.shape
    sizes = np.asarray(sizes, dtype=np.int64)
    bases = np.asarray(bases, dtype=np.int64)
    valid = li >= 0
    gi = bases[:, None] + li
    key = (v & np.uint32(0x7FFFFFFF)).astype(np.int64)
    flat = np.nonzero(valid.ravel())[0]
    if sel is None:
        order = np.lexsort((gi.ravel()[flat], -key.ravel()[flat]))
        sel = np.zeros(world * cap, dtype=bool)
        sel[flat[order[:min(int(k), flat.size)]]] = True
        sel = sel.reshape(world, cap)
    sel_gi = np.where(sel, gi, -1).astype(np.int32)
    out = np.zeros(int(out_len), dtype=np.float32)
    q = gi[sel] - int(out_base)
    ok = (q >= 0) & (q < int(out_len))
    with np.errstate(invalid="ignore"):
        out[q[ok]] = np.float32(0.0) + v.view(np.float32)[sel][ok]
    rej = valid[rank] & ~sel[rank]
    status = (1 if np.any(np.asarray(hdr_m, dtype=np.int64) != sizes) else 0) | (2 if flat.size < int(k) else 0)
    return {"sel": sel, "sel_gi": sel_gi.ravel(), "pay_idx": sel_gi[rank].copy(), "out_f32": out,
            "out_pos": q[ok], "restore": (li[rank][rej], v[rank][rej]), "status": status}


# ------------------------------------------------------------------------------- the model
def _bin_desc(hist, rank):
    """the bin d with sum(hist[d+1:]) < rank <= sum(hist[d:]) and the count above it; BINS for
    rank 0, -1 when the histogram holds fewer than `rank`"""
    total = int(hist.sum())
    if rank == 0:
        return len(hist), total
    if total < rank:
        return -1, total
    run = np.cumsum(hist[::-1])
    d = len(hist) - 1 - int(np.searchsorted(run, rank, side="left"))
    return d, int(hist[d + 1:].sum())


def _radix_passes(comp, need):
    """passes (11/11/11/11/11/9 bits from the top) the single-workgroup radix select runs until the
    chosen digit's bin holds exactly what is still needed"""
    comp = np.asarray(comp, dtype=np.uint64)
    live = np.ones(comp.size, dtype=bool)
    rem = int(need)
    for p in range(6):
        shift, mask = (53 - 11 * p, 2047) if p < 5 else (0, 511)
        dig = ((comp >> np.uint64(shift)) & np.uint64(mask)).astype(np.int64)
        hist = np.bincount(dig[live], minlength=2048)
        d, above = _bin_desc(hist, rem)
        rem -= above
        live &= dig == d
        if int(hist[d]) == rem:
            return p + 1
    return 6


def branch_model(vals_u32, li, bases, k):
    """The kernel's bookkeeping for these records and this k (see the module docstring)."""
    v = np.ascontiguousarray(vals_u32, dtype=np.uint32)
    li = np.asarray(li, dtype=np.int64)
    world, cap = v.shape
    n = world * cap
    valid = (li >= 0).ravel()
    key = (v & np.uint32(0x7FFFFFFF)).ravel()
    coarse = (key >> np.uint32(20)).astype(np.int64)
    sub = ((key >> np.uint32(9)) & np.uint32(BINS - 1)).astype(np.int64)
    c1, above = _bin_desc(np.bincount(coarse[valid], minlength=BINS), int(k))
    need = 0 if c1 < 0 else int(k) - above
    in_c1 = valid & (coarse == c1)
    nblk = (n + LIST_BLOCK - 1) // LIST_BLOCK
    block_counts = np.add.reduceat(in_c1.astype(np.int64), np.arange(0, n, LIST_BLOCK))
    b2, above2 = _bin_desc(np.bincount(sub[in_c1], minlength=BINS), need)
    cut = in_c1 & (sub == b2)
    need2 = need - above2 if 0 <= b2 < BINS else 0
    n2 = int(cut.sum())
    path = "pairwise" if n2 <= PAIR_CAP else "radix"
    passes = 0
    if path == "radix":
        gi = (np.asarray(bases, dtype=np.int64)[:, None] + li).ravel()[cut]
        comp = (key[cut].astype(np.uint64) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - gi.astype(np.uint64))
        passes = _radix_passes(comp, need2)
    grid = max(1, min(MAX_GRID, nblk))
    return {"n": n, "valid": int(valid.sum()), "c1": c1, "c1_count": int(in_c1.sum()), "need": need,
            "block_counts": block_counts, "b2": b2, "need2": need2, "n2": n2, "path": path,
            "radix_passes": passes,
            # passes 0 .. 2 hold the 32 key bits (and index bit 31); a fourth pass is index digits only
            "index_digits": passes >= 4,
            "nblk": nblk, "grid": grid, "rounds": (nblk + grid - 1) // grid,
            "shared_copy": grid > GROUPS}


# ------------------------------------------------------------------------------- builders
def deal(patterns, world, cap, counts=None, signs=True):
    """Deal the value bit patterns over ranks and slots: entry i goes to the i-th (slot, rank) pair
    in slot-major order among the ranks that still have room (counts[w] valid entries, default
    full), so neighbours in `patterns` sit on different ranks.  A rank's slots hold DESCENDING local
    indices 3 (m - 1 - c) + (world - 1 - w) % 3 (a later slot and a higher rank's offset win a tie
    inside a shard's range; the global order is the rank's base first), shards are 3 counts[w] + 5
    long, and every third entry is negated (-v and +v share a key).  Padding slots hold PAD_BITS
    and local index -1.  Returns (vals_u32[W, cap], li[W, cap], sizes)."""
    patterns = np.asarray(patterns, dtype=np.uint32)
    counts = np.full(world, cap, dtype=np.int64) if counts is None else np.asarray(counts, dtype=np.int64)
    assert counts.shape == (world,) and counts.max() <= cap and counts.sum() == patterns.size
    room = np.arange(cap)[:, None] < counts[None, :]            # [slot, rank]
    c, w = np.nonzero(room)                                     # slot-major
    p = patterns.copy()
    if signs:
        p[1::3] ^= np.uint32(0x80000000)
    vals = np.full((world, cap), PAD_BITS, dtype=np.uint32)
    li = np.full((world, cap), -1, dtype=np.int32)
    vals[w, c] = p
    li[w, c] = 3 * (counts[w] - 1 - c) + (world - 1 - w) % 3
    return vals, li, [int(3 * m + 5) for m in counts]


def bases_of(sizes):
    return [int(sum(sizes[:r])) for r in range(len(sizes))]


def _spread(counts_total, world, cap, short=()):
    """per-rank valid counts summing to counts_total: the ranks in `short` (a dict rank -> count)
    as given, the rest as even as possible within cap"""
    counts = np.zeros(world, dtype=np.int64)
    free = [r for r in range(world) if r not in dict(short)]
    for r, m in dict(short).items():
        counts[r] = m
    left = counts_total - int(counts.sum())
    for i, r in enumerate(free):
        counts[r] = left // len(free) + (1 if i < left % len(free) else 0)
    assert counts.max() <= cap and counts.sum() == counts_total, (counts_total, world, cap)
    return counts


def cut_population(T, need2, world=3, H=5, n7=6, n1=4, nbelow=7, seed=1):
    """T entries in sub-bin 3 of C1 around the cut: H entries above C1, n7 in sub-bin 7, n1 in
    sub-bin 1, nbelow below C1; k = H + n7 + need2 puts the cut need2 entries into sub-bin 3.  The
    low bits are i % 512: distinct keys while T <= 512, repeated keys (ranked by global index)
    beyond.  Returns (vals, li, sizes, k)."""
    i = np.arange(T, dtype=np.uint32)
    pats = np.concatenate([
        ABOVE_BITS | (np.arange(H, dtype=np.uint32) * np.uint32(0x20003)),
        C1_BITS | np.uint32(7 << 9) | np.arange(n7, dtype=np.uint32),
        C1_BITS | np.uint32(3 << 9) | (i % np.uint32(512)),
        C1_BITS | np.uint32(1 << 9) | np.arange(n1, dtype=np.uint32),
        BELOW_BITS | (np.arange(nbelow, dtype=np.uint32) * np.uint32(1001)),
    ]).astype(np.uint32)
    pats = pats[np.random.default_rng(seed).permutation(pats.size)]
    cap = (pats.size + world - 1) // world + 2                  # every rank ends on pads
    vals, li, sizes = deal(pats, world, cap, _spread(pats.size, world, cap))
    return vals, li, sizes, H + n7 + need2


def identical(n, world, bits=0x3F800000, mixed_sign=False):
    """n = world * cap valid entries, all of one bit pattern (mixed_sign: every third negated, as
    +0 / -0): the order is the global index alone"""
    assert n % world == 0
    return deal(np.full(n, bits, dtype=np.uint32), world, n // world, signs=mixed_sign)


def mixed(world, cap, counts, seed):
    """valid entries drawn from a small pool with many repeats: above C1, sub-bins 7 / 3 / 1 of C1
    with four low-bit values each, below C1"""
    pool = np.concatenate([
        ABOVE_BITS | np.arange(3, dtype=np.uint32),
        (C1_BITS | (np.array([7, 3, 3, 3, 1], dtype=np.uint32)[:, None] << np.uint32(9))
         | np.arange(4, dtype=np.uint32)[None, :]).ravel(),
        BELOW_BITS | np.arange(5, dtype=np.uint32),
    ]).astype(np.uint32)
    rng = np.random.default_rng(seed)
    counts = np.asarray(counts, dtype=np.int64)
    return deal(pool[rng.integers(0, pool.size, int(counts.sum()))], world, cap, counts)


def two_maxima():
    """world 3, cap 4: the maximum 0x40400000 twice, once in rank 2 (slot 0) and once in rank 1
    (its LAST slot); k = 1 must take rank 1's, the lower global index"""
    pats = np.array([0x3F800000, 0x3F800001, 0x40400000,    # slot 0 of ranks 0, 1, 2
                     0x3F800002, 0x3F000000, 0x3F800003,
                     0x3F800004, 0x40400000, 0x3F800005], dtype=np.uint32)
    return deal(pats, 3, 4, [3, 3, 3], signs=False)


def special_patterns():
    """about 200 patterns: NaNs of several payloads, inf, the largest finite values, zero,
    subnormals, and neighbours differing in the last bit at every bin edge -- each with both signs"""
    pos = [0x7FC00000, 0x7FC00001, 0x7FFFFFFF, 0x7F800001, 0x7FA00000, 0x7FBFFFFF, 0x7FFFFFFE, 0x7FC12345,
           0x7F800000, 0x7F7FFFFF, 0x7F7FFFFE, 0x7F000000,
           0x00000000, 0x00000001, 0x00000002, 0x000001FF, 0x00000200, 0x00000201, 0x00400000, 0x007FFFFF,
           0x00800000, 0x00800001, 0x000FFFFF, 0x00100000,
           0x3F7FFFFF, 0x3F800000, 0x3F800001, 0x3F8001FF, 0x3F800200, 0x3F800201, 0x3F8FFFFF, 0x3F900000,
           0x3F900001, 0x3FFFFFFF, 0x40000000, 0x40000001]
    for e in (1, 2, 64, 100, 126, 127, 128, 129, 200, 253, 254):
        for m in (0, 1, 0x1FF, 0x200, 0x0FFFFF, 0x100000, 0x7FFFFE, 0x7FFFFF):
            pos.append((e << 23) | m)
    pos = np.unique(np.array(pos, dtype=np.uint32))
    return np.concatenate([pos, pos | np.uint32(0x80000000)])


def special_values(world=2, seed=3):
    pats = special_patterns()
    pats = pats[np.random.default_rng(seed).permutation(pats.size)]
    cap = (pats.size + world - 1) // world + 3
    return deal(pats, world, cap, _spread(pats.size, world, cap), signs=False)


def layout(world, cap, seed):
    """world * cap slots of mixed entries; for world > 1 one rank holds a single valid entry and
    every third other rank ends on pads"""
    counts = np.full(world, cap, dtype=np.int64)
    if world > 1:
        counts[1::3] = np.maximum(1, cap - 1 - (np.arange(world)[1::3] % max(1, cap // 2)))
        counts[world // 2] = 1
    return mixed(world, cap, counts, seed)


def large(world=513, cap=4096, seed=7):
    """2.1 M entries, every key in C1, sub-bins and low bits uniform: 513 list blocks on a grid of
    512"""
    rng = np.random.default_rng(seed)
    n = world * cap
    pats = (np.uint32(C1_BITS) | (rng.integers(0, BINS, n).astype(np.uint32) << np.uint32(9))
            | rng.integers(0, 512, n).astype(np.uint32))
    return deal(pats, world, cap)


# ------------------------------------------------------------------------------- the cases
def _cut_cases():
    out = {}
    for T in (1, 1023, 1024, 1025, 3000):
        for need2 in sorted({1, max(1, T // 2), max(1, T - 1), T}):
            out[f"cut-T{T}-need{need2}"] = {
                "build": (cut_population, (T, need2)),
                "expect": {"c1": C1_BIN, "b2": 3, "n2": T, "need2": need2, "need": 6 + need2,
                           "path": "pairwise" if T <= PAIR_CAP else "radix", "nblk": 1}}
    return out


def _identical_cases():
    out = {}
    for tag, bits, mixed_sign in (("one", 0x3F800000, False), ("zero", 0x00000000, True)):
        for n, world in ((4096, 4), (9 * 4096 + 1, 5)):
            for k in (1, n // 2, n - 1):
                out[f"same-{tag}-n{n}-k{k}"] = {
                    "build": (identical, (n, world, bits, mixed_sign)), "k": k,
                    "expect": {"n": n, "valid": n, "n2": n, "need2": k, "path": "radix", "index_digits": True,
                               "radix_passes": 6, "shared_copy": n > 8 * LIST_BLOCK}}
    return out


CASES = {}
CASES.update(_cut_cases())
CASES.update(_identical_cases())
CASES.update({
    # ---- k edges
    "k1-two-maxima": {"build": (two_maxima, ()), "k": 1,
                      "expect": {"c1": 0x40400000 >> 20, "need": 1, "c1_count": 2, "n2": 2, "need2": 1,
                                 "path": "pairwise"}},
    "k-valid": {"build": (mixed, (3, 40, [40, 17, 1], 11)), "k": 58,
                "expect": {"valid": 58, "c1": BELOW_BITS >> 20, "need_whole_c1": True}},
    "k-valid+1": {"build": (mixed, (3, 40, [40, 17, 1], 11)), "k": 59,
                  "expect": {"valid": 58, "c1": -1, "need": 0, "b2": BINS, "n2": 0, "status": 2}},
    "cap3000-k10": {"build": (mixed, (2, 3000, [3000, 50], 12)), "k": 10,
                    "expect": {"n": 6000, "nblk": 2, "c1": ABOVE_BITS >> 20, "path": "pairwise"}},
    "w64-cap100-k5000": {"build": (mixed, (64, 100, [100 - (r % 5) for r in range(64)], 13)), "k": 5000,
                         "expect": {"n": 6400, "valid": 6274, "nblk": 2, "c1": C1_BIN, "b2": 1, "path": "pairwise"}},
    # ---- layout
    "layout-w1-n4096": {"build": (layout, (1, 4096, 21)), "k": 2000, "expect": {"n": 4096, "nblk": 1, "grid": 1}},
    "layout-w1-n4097": {"build": (layout, (1, 4097, 22)), "k": 2000, "expect": {"n": 4097, "nblk": 2, "grid": 2}},
    "layout-w2-n8x4096": {"build": (layout, (2, 4 * 4096, 23)), "k": 9000,
                          "expect": {"n": 8 * 4096, "nblk": 8, "shared_copy": False}},
    "layout-w5-n9x4096+1": {"build": (layout, (5, 7373, 24)), "k": 7373,
                            "expect": {"n": 9 * 4096 + 1, "nblk": 10, "shared_copy": True}},
    "layout-w7": {"build": (layout, (7, 586, 25)), "k": 586, "expect": {"n": 4102, "nblk": 2}},
    "layout-w64-n4096": {"build": (layout, (64, 64, 26)), "k": 700, "expect": {"n": 4096, "nblk": 1}},
    "layout-w1024-cap5": {"build": (layout, (1024, 5, 27)), "k": 1500, "expect": {"n": 5120, "nblk": 2}},
    # ---- large
    "large-w513": {"build": (large, ()), "k": 513 * 4096 // 2,
                   "expect": {"n": 513 * 4096, "nblk": 513, "grid": 512, "rounds": 2, "c1": C1_BIN,
                              "c1_count": 513 * 4096}},
    # ---- special values (the k sweep runs every k in 1 .. valid + 1; the model is asserted at k = valid / 2)
    "special": {"build": (special_values, ()), "k": None, "expect": {"nblk": 1}},
    # ---- windows and status run on a small cut population
    "window-base": {"build": (cut_population, (40, 20)), "expect": {"b2": 3, "n2": 40, "need2": 20,
                                                                    "path": "pairwise"}},
})


def build_case(name):
    """(vals, li, sizes, k, expect) of a CASES entry"""
    c = CASES[name]
    fn, args = c["build"]
    got = fn(*args)
    if len(got) == 4:
        vals, li, sizes, k = got
    else:
        (vals, li, sizes), k = got, c["k"]
    return vals, li, sizes, k, c["expect"]


def check_model(name, vals, li, sizes, k, expect):
    """assert that branch_model reports the branch the case is named after; returns the model"""
    m = branch_model(vals, li, bases_of(sizes), k)
    for key, want in expect.items():
        if key == "status":
            continue
        if key == "need_whole_c1":
            assert (m["need"] == m["c1_count"] and m["n2"] == m["need2"]) == want, (name, key, m)
            continue
        assert m[key] == want, (name, key, m[key], want)
    gi = (np.asarray(bases_of(sizes), dtype=np.int64)[:, None] + li)[li >= 0]
    assert np.unique(gi).size == gi.size, name      # unique global indices
    return m
