"""DGC's threshold engine (grace_amd/csrc/dgc.hip) against the oracle where its own design can go
wrong: the tabulated adjustment loop (dgc_table_kernel, dgc_count_kernel through tab_bin_lut,
dgc_replay_kernel) on inputs that take the reference's loop (dgc.py:28-36) down long and mixed
paths, with ties on table values, thresholds of 0, inf, near FLT_MAX and subnormal; lengths around
the 4,096-element compaction chunk and the 16,384-element world-1 chunk, below 100 elements,
4-byte-misaligned buffers (the scalar paths) and tensors past one trip of the capped grids; and
three-step momentum chains.  Every case runs through the three entries that share the engine --
dgc_compress, dgc_select + dgc_step_w1, and the one-pass dgc_step_w1_fused with its gated fix-up --
and is compared bit for bit with oracle/grace_oracle.py (payload, threshold, count, out, r', a').
Each loop case first asserts on the CPU that the oracle takes the path it was built for."""
import numpy as np
import pytest
import torch

from grace_amd import ops
from oracle import grace_oracle as O
from tests.dgc_edge_util import LOOP_CASES, alternations, bits, ns_of
from tests.golden_util import same_bits

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = np.float32

# launch geometry of dgc.hip (kDBlock threads, kDQ quads of 4 per thread per round)
K_BLOCK, K_DQ, K_CHUNK, K_CHUNK_W1 = 256, 4, 4096, 16384
COUNT_CAP, FIXUP_CAP = 2048, 1024           # stream_grid caps of grace_dgc_threshold / the fused fix-up


def _t(a, misalign=False):
    """a on the device; misalign: as the view buf[1:] of a 16-byte-aligned buffer (4 bytes off)."""
    src = torch.from_numpy(np.ascontiguousarray(a))
    if not misalign:
        return src.to(DEV)
    buf = torch.empty(src.numel() + 1, dtype=src.dtype, device=DEV)
    view = buf[1:]
    view.copy_(src)
    assert buf.data_ptr() % 16 == 0 and view.data_ptr() % 16 == 4 and view.is_contiguous()
    return view


def _np(t):
    return t.detach().cpu().numpy()


def _meta_words(meta):
    """(thr bits, count) of a DGC workspace's leading meta words {thr0, thr, count, nan0}."""
    w = _np(meta[:16].view(torch.int32)).view(np.uint32)
    return int(w[1]), int(w[2])


def _w1_meta():
    return _meta_words(ops.workspace("dgc_w1", 1, torch.device(DEV, torch.cuda.current_device())))


def _oracle_step(g, r, a, momentum, sidx, ratio):
    """Allgather(DgcCompressor, DgcMemory, 1).step on the CPU: compensate, compress, update and
    (0 + decompress) / 1; r = a = None on a name's first step."""
    with np.errstate(invalid="ignore", over="ignore"):
        t, rc, ac = O.dgc_memory_compensate(g, r, a, momentum)
        vals, idx, mask, thr = O.dgc_compress(t, sidx, ratio)
        rn, an = O.dgc_memory_update(rc, ac, mask)
        dec = O.sparse_decode(vals, idx, t.size)
        out = (O.python_sum([dec]) / F32(1)).astype(F32)
    return dict(t=t, vals=vals, idx=idx, mask=mask, thr=bits(thr), total=int(idx.size), dec=dec, out=out, r=rn,
                a=an)


def _same(got, want, what):
    got = _np(got)
    if not same_bits(got, want):
        bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
        raise AssertionError(f"{what}: {bad.size} of {want.size} differ, first at {bad[:5]}: "
                             f"got {got[bad[:5]]}, want {want[bad[:5]]}")


def _check_first_step(x, sidx, ratio, what, misalign=False):
    """x through the three entries as a first step, everything against the oracle."""
    n = x.size
    e = _oracle_step(x, None, None, 0.9, sidx, ratio)
    sd = _t(sidx)
    r0 = np.random.default_rng(n).standard_normal(n).astype(F32)     # a residual unlike x: multiplied, not copied
    with np.errstate(invalid="ignore"):
        er0 = O.dgc_memory_update(r0, x, e["mask"])[0]

    # grace_dgc_threshold + grace_dgc_write, then the mask update and the decode of that payload
    xd = _t(x, misalign)
    vals, idx, meta = ops.dgc_compress(xd, ratio, sample_idx=sd)
    assert _meta_words(meta) == (e["thr"], e["total"]), (what, "compress", _meta_words(meta), e["thr"], e["total"])
    assert idx.dtype == torch.int64 and np.array_equal(_np(idx), e["idx"]), (what, "compress idx")
    _same(vals, e["vals"], f"{what}: compress values")
    _same(ops.sparse_decode(vals, idx, n), e["dec"], f"{what}: decode")
    r, a = _t(r0), _t(x, misalign)
    ops.dgc_mask_update(a, r, a, meta)
    _same(r, er0, f"{what}: mask_update r")
    _same(a, e["a"], f"{what}: mask_update a")

    # grace_dgc_select + grace_dgc_step_w1
    r, a = _t(r0), _t(x, misalign)
    ws = ops.dgc_select(a, ratio, sample_idx=sd)
    assert _meta_words(ws) == (e["thr"], e["total"]), (what, "select", _meta_words(ws), e["thr"], e["total"])
    out = ops.dgc_step_w1(a, r, a, ws)
    _same(out, e["out"], f"{what}: step_w1 out")
    _same(r, er0, f"{what}: step_w1 r")
    _same(a, e["a"], f"{what}: step_w1 a")

    # grace_dgc_sample_comp + grace_dgc_step_w1_fused, first step (r' = a' = g * keep)
    out, rn, an = ops.dgc_step_w1_fused(_t(x, misalign), None, None, False, 0.9, ratio, sample_idx=sd)
    assert _w1_meta() == (e["thr"], e["total"]), (what, "fused", _w1_meta(), e["thr"], e["total"])
    _same(out, e["out"], f"{what}: fused out")
    _same(rn, e["r"], f"{what}: fused r")
    _same(an, e["a"], f"{what}: fused a")
    return e


# ------------------------------------------------------------------------------------------------
# A. the adjustment loop
@pytest.mark.parametrize("name", sorted(LOOP_CASES))
def test_dgc_adjustment_loop_vs_oracle(name):
    case = LOOP_CASES[name]()
    trace = case.check_path()                       # the oracle takes the path this input was built for
    e = _check_first_step(case.x, case.sidx, case.ratio, name)
    assert e["thr"] == bits(trace[-1][1]) and e["total"] == trace[-1][2]


def _random_case(n, seed, scale_tail=0):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(n).astype(F32)
    if scale_tail:
        x[n - scale_tail:] *= F32(1e-3)
    return x, rng.integers(0, n, ns_of(n)).astype(np.int64)


@pytest.mark.parametrize("n", [K_CHUNK - 1, K_CHUNK, K_CHUNK + 1, K_CHUNK_W1 - 1, K_CHUNK_W1, K_CHUNK_W1 + 1,
                               3 * K_CHUNK_W1 + 5])
def test_dgc_chunk_edges_vs_oracle(n):
    """Lengths around the compaction chunk and the world-1 chunk; at 3 chunks + 5 the last chunk
    of both (5 small elements) contributes nothing to the payload."""
    tail = n % K_CHUNK_W1 if n > 3 * K_CHUNK_W1 else 0
    x, sidx = _random_case(n, n, scale_tail=tail)
    e = _check_first_step(x, sidx, 0.01, f"n={n}")
    assert e["total"] > 0
    if tail:
        assert tail == 5 and e["idx"].max() < n - tail


@pytest.mark.parametrize("sample", ["random", "largest"])
def test_dgc_misaligned_first_step_vs_oracle(sample):
    """A 4-byte-misaligned input: dgc_count_kernel, dgc_mask_kernel and dgc_w1_spec_kernel take their
    scalar paths; with the largest element sampled the loop and the fused step's fix-up run."""
    n = K_CHUNK_W1 + 1 + 2
    x, sidx = _random_case(n, 77)
    if sample == "largest":
        sidx[:] = int(np.argmax(np.abs(x)))
        assert "D" in O.dgc_adjust_path(x, sidx, 0.01)
    _check_first_step(x, sidx, 0.01, f"misaligned {sample}", misalign=True)


@pytest.mark.parametrize("sample", ["random", "largest"])
@pytest.mark.parametrize("which", ["g", "ra"])
def test_dgc_fused_misaligned_second_step_vs_oracle(which, sample):
    """The fused step with carried state when g alone, or (r, a) alone, is 4 bytes off alignment."""
    n, ratio, m = K_CHUNK_W1 + 1 + 2, 0.01, 0.9
    rng = np.random.default_rng(5)
    g1, g2 = rng.standard_normal(n).astype(F32), rng.standard_normal(n).astype(F32)
    s1 = rng.integers(0, n, ns_of(n)).astype(np.int64)
    e1 = _oracle_step(g1, None, None, m, s1, ratio)
    t2 = O.dgc_memory_compensate(g2, e1["r"], e1["a"], m)[0]
    s2 = rng.integers(0, n, ns_of(n)).astype(np.int64)
    if sample == "largest":
        s2[:] = int(np.argmax(np.abs(t2)))
        assert "D" in O.dgc_adjust_path(t2, s2, ratio)
    e2 = _oracle_step(g2, e1["r"], e1["a"], m, s2, ratio)
    out, r, a = ops.dgc_step_w1_fused(_t(g1), None, None, False, m, ratio, sample_idx=_t(s1))
    _same(out, e1["out"], "step 1 out")
    _same(r, e1["r"], "step 1 r")
    _same(a, e1["a"], "step 1 a")
    gd = _t(g2, misalign=which == "g")
    if which == "ra":
        r, a = _t(_np(r), misalign=True), _t(_np(a), misalign=True)
    out, rn, an = ops.dgc_step_w1_fused(gd, r, a, True, m, ratio, sample_idx=_t(s2))
    assert _w1_meta() == (e2["thr"], e2["total"])
    _same(out, e2["out"], f"{which} {sample}: out")
    _same(rn, e2["r"], f"{which} {sample}: r")
    _same(an, e2["a"], f"{which} {sample}: a")
    _same(r, e1["r"], "the old residual is only read")
    _same(a, e1["a"], "the old accumulator is only read")


def test_dgc_past_one_trip_of_the_count_grid_vs_oracle():
    """grace_dgc_threshold counts on at most COUNT_CAP workgroups of K_BLOCK threads, K_DQ quads
    per thread per round: one more element than a round holds, and not a multiple of 4, sends
    every workgroup round the loop again (the quads of the second round, then the scalar tail)."""
    trip = COUNT_CAP * K_BLOCK * K_DQ * 4
    n = trip + K_CHUNK + 3
    assert n % 4 and (n + 3) // 4 > COUNT_CAP * K_BLOCK * K_DQ
    x, sidx = _random_case(n, 11)
    x[trip:] *= F32(3)                         # the second trip's elements weigh in the counts
    e = _check_first_step(x, sidx, 0.01, "count grid")
    assert (e["idx"] >= trip).sum() > 100


def test_dgc_past_one_trip_of_the_fixup_grid_vs_oracle():
    """The fused step's gated fix-up (compensate, count, mask) runs on at most FIXUP_CAP
    workgroups; the largest element is sampled so that thr0 cannot stand and the fix-up runs."""
    trip = FIXUP_CAP * K_BLOCK * K_DQ * 4
    n = trip + K_CHUNK + 3
    assert n % 4 and (n + 3) // 4 > FIXUP_CAP * K_BLOCK * K_DQ
    x, sidx = _random_case(n, 12)
    x[trip:] *= F32(3)
    sidx[:] = int(np.argmax(np.abs(x)))
    path = O.dgc_adjust_path(x, sidx, 0.01)
    assert len(path) >= 2 and path[0] == "D", path
    e = _check_first_step(x, sidx, 0.01, "fix-up grid")
    assert (e["idx"] >= trip).sum() > 100


# ------------------------------------------------------------------------------------------------
# B. momentum chains
def _chain_inputs():
    """Three gradients and samples at n = 40003: step 1 selects a +inf and a -inf (r' = a' = NaN
    there from then on), step 2 carries a NaN gradient entry and samples the 400 smallest
    magnitudes of its compensated tensor (ten ups), step 3 samples one element high in the tail
    (a mixed path): the oracle's steps, with each path's property asserted."""
    n, ratio, m = 40000 + 3, 0.01, 0.9
    rng = np.random.default_rng(21)
    gs = [rng.standard_normal(n).astype(F32) for _ in range(3)]
    gs[0][[100, 20000]] = [np.inf, -np.inf]
    gs[1][30000] = np.nan
    steps, r, a = [], None, None
    for s in range(3):
        t = O.dgc_memory_compensate(gs[s], r, a, m)[0]
        order = np.argsort(np.abs(t), kind="stable")          # NaN last
        valid = order[:n - int(np.isnan(t).sum())]
        if s == 0:
            sidx = rng.choice(valid, ns_of(n))
        elif s == 1:
            sidx = valid[:ns_of(n)]
        else:
            sidx = np.full(ns_of(n), valid[int(0.985 * valid.size)])
        sidx = sidx.astype(np.int64)
        path = O.dgc_adjust_path(t, sidx, ratio)
        if s == 1:
            assert path == "U" * 10, path
        if s == 2:
            assert len(path) >= 3 and alternations(path) >= 1, path
        e = _oracle_step(gs[s], r, a, m, sidx, ratio)
        e["g"], e["sidx"], e["path"] = gs[s], sidx, path
        steps.append(e)
        r, a = e["r"], e["a"]
    # what the chain was built to carry: -0 and NaN in the masked memory, a NaN that stays
    assert np.isnan(steps[0]["r"][[100, 20000]]).all() and np.isnan(steps[2]["a"][[100, 20000, 30000]]).all()
    for e in steps:
        sel = e["idx"][np.isfinite(e["vals"]) & (e["vals"] < 0)]
        assert sel.size and np.signbit(e["a"][sel]).all() and (e["a"][sel] == 0).all()
        assert np.signbit(e["r"][e["idx"]]).any() and not np.signbit(e["r"][e["idx"]]).all()
    return n, ratio, m, steps


@pytest.fixture(scope="module")
def chain():
    return _chain_inputs()


def test_dgc_fused_momentum_chain_vs_oracle(chain):
    n, ratio, m, steps = chain
    r = a = None
    for s, e in enumerate(steps):
        out, r, a = ops.dgc_step_w1_fused(_t(e["g"]), r, a, s > 0, m, ratio, sample_idx=_t(e["sidx"]))
        assert _w1_meta() == (e["thr"], e["total"]), (s, e["path"])
        _same(out, e["out"], f"step {s} ({e['path']}): out")
        _same(r, e["r"], f"step {s} ({e['path']}): r")
        _same(a, e["a"], f"step {s} ({e['path']}): a")


def test_dgc_multipass_momentum_chain_vs_oracle(chain):
    n, ratio, m, steps = chain
    r, a = torch.empty(n, dtype=torch.float32, device=DEV), torch.empty(n, dtype=torch.float32, device=DEV)
    for s, e in enumerate(steps):
        ops.dgc_compensate(_t(e["g"]), r, a, s > 0, m)
        _same(a, e["t"], f"step {s}: compensated tensor")
        ws = ops.dgc_select(a, ratio, sample_idx=_t(e["sidx"]))
        assert _meta_words(ws) == (e["thr"], e["total"]), (s, e["path"])
        out = ops.dgc_step_w1(a, r, a, ws)
        _same(out, e["out"], f"step {s} ({e['path']}): out")
        _same(r, e["r"], f"step {s} ({e['path']}): r")
        _same(a, e["a"], f"step {s} ({e['path']}): a")


# ------------------------------------------------------------------------------------------------
# C. the three-digit radix select against torch.topk(x, ks)[0].min()
K_KTH_TILE, K_KTH_GRID = 4096, 1024          # elements per workgroup per round, workgroups at most
KTH_DIGITS = ((20, 2048), (9, 2048), (0, 512))     # (shift, bins) of the digits, most significant first


def _kth_check(x, ks, what, xd=None):
    want = torch.topk(torch.from_numpy(x), ks)[0].min().reshape(1).numpy()
    got = _np(ops.dgc_sample_kth(_t(x) if xd is None else xd, ks))
    if np.isnan(want[0]):
        # torch's min returns whichever NaN its reduction order meets or makes (0x7FC00000 at one
        # rank, 0xFFFFFFFF at another, for the same input): a NaN for a NaN, the engine's is quiet
        assert got.view(np.uint32)[0] == 0x7FC00000, (what, ks, got.view(np.uint32))
        return want
    assert same_bits(got, want), (what, ks, got, want, got.view(np.uint32), want.view(np.uint32))
    return want


@pytest.mark.parametrize("ns", [1, 255, 256, K_KTH_TILE - 1, K_KTH_TILE, K_KTH_TILE + 1])
def test_dgc_kth_sizes_around_the_workgroup_tile(ns):
    x = np.abs(np.random.default_rng(ns).standard_normal(ns)).astype(F32)
    xd = _t(x)
    for ks in sorted({1, (ns + 1) // 2, ns}):
        _kth_check(x, ks, f"ns={ns}", xd)
    x[ns - 1] = np.nan                          # the last element of the tile: NaN wins at every rank
    for ks in sorted({1, ns}):
        assert np.isnan(_kth_check(x, ks, f"ns={ns} nan")[0])


def _digit_keys(level, d, ns, rng):
    """ns magnitude keys whose digit `level` takes values around d while every more significant
    digit is shared (0x3F8 above the middle digit, 5 in the middle digit above the last)."""
    shift, nbins = KTH_DIGITS[level]
    top = 2039 if level == 0 else nbins - 1                # 2039: the largest finite exponent digit
    dig = rng.integers(max(0, d - 2), min(top, d + 2) + 1, ns).astype(np.uint32)
    dig[:8] = d
    low = rng.integers(0, 1 << shift, ns).astype(np.uint32) if shift else np.zeros(ns, np.uint32)
    high = np.uint32(0 if level == 0 else (0x3F800000 if level == 1 else 0x3F800000 | (5 << 9)))
    key = high | (dig << np.uint32(shift)) | low
    assert (key <= 0x7F800000).all()
    return key


@pytest.mark.parametrize("level,d", [(lv, d) for lv in (0, 1) for d in (0, 31, 32, 33, "top")] +
                         [(2, d) for d in (0, 7, 8, 9, "top")])
def test_dgc_kth_decides_in_each_digit_at_lane_boundaries(level, d):
    """The answer's digit `level` is d with the digits above it decided by a single bin: bin 0, the
    lane boundaries of the last arriver's walk (32 bins per lane in the 2,048-bin digits, 8 in the
    512-bin digit) and the top bin; at the smallest key of the bin (the rank uses the whole bin)
    and at its largest (rank 1 within the bin)."""
    shift, nbins = KTH_DIGITS[level]
    d = (2039 if level == 0 else nbins - 1) if d == "top" else d      # 2039: the largest finite exponent digit
    ns = 2 * K_KTH_TILE + 17
    key = _digit_keys(level, d, ns, np.random.default_rng(100 * level + d))
    x = key.view(F32)
    xd = _t(x)
    in_bin = key[((key >> np.uint32(shift)) & np.uint32(nbins - 1)) == d]
    for target in sorted({int(in_bin.min()), int(in_bin.max())}):
        ks = int((key >= target).sum())
        want = _kth_check(x, ks, f"level {level} digit {d}", xd)
        assert int(want.view(np.uint32)[0]) == target
    if d > 0:                                   # one rank further: the walk leaves the bin for the one below
        ks = int((key >= int(in_bin.min())).sum()) + 1
        want = _kth_check(x, ks, f"level {level} below digit {d}", xd)
        assert ((int(want.view(np.uint32)[0]) >> shift) & (nbins - 1)) < d


def test_dgc_kth_every_key_of_the_last_digit():
    """0x3F800000 | 0..511, 17 copies of each, shuffled: the first two digits are decided by a
    single bin and every rank's answer by the 9-bit digit alone -- the rank that ends a bin, the
    one that starts the next, and one inside, at bin 0, the 8-bin lane boundaries and the top."""
    reps = 17
    key = np.tile(np.uint32(0x3F800000) | np.arange(512, dtype=np.uint32), reps)
    np.random.default_rng(6).shuffle(key)
    x = key.view(F32)
    xd = _t(x)
    for d in (0, 1, 7, 8, 9, 255, 256, 510, 511):
        above = (511 - d) * reps                # keys larger than 0x3F800000 | d
        for ks in (above + 1, above + reps // 2, above + reps):
            want = _kth_check(x, ks, f"last digit {d}", xd)
            assert int(want.view(np.uint32)[0]) == 0x3F800000 | d, (d, ks)


def test_dgc_kth_answer_in_bin_zero():
    """Mostly zeros with c non-zeros: a rank past c is 0.0 (bin 0 of every digit), rank c is not."""
    ns, c = 5000, 37
    rng = np.random.default_rng(9)
    x = np.zeros(ns, dtype=F32)
    x[rng.choice(ns, c, replace=False)] = np.abs(rng.standard_normal(c)).astype(F32) + F32(0.5)
    xd = _t(x)
    assert _kth_check(x, c, "rank c", xd)[0] >= 0.5
    for ks in (c + 1, ns // 2, ns):
        assert bits(_kth_check(x, ks, "past c", xd)[0]) == 0


def test_dgc_kth_grid_stride_and_state_across_sizes():
    """More workgroups' worth than the 1,024-workgroup grid (a second trip for the first
    workgroups), then a small sample, then the large one again at other ranks: the shared
    workspace is left zeroed by every call."""
    ns = K_KTH_GRID * K_KTH_TILE + 5
    gen = torch.Generator().manual_seed(3)
    big = torch.randn(ns, generator=gen).abs().numpy()
    big[ns - 3:] = [7.5, 0.0, 9.25]             # the second trip's elements hold the top two ranks
    small = np.abs(np.random.default_rng(4).standard_normal(255)).astype(F32)
    bd = _t(big)
    assert _kth_check(big, 2, "big ks=2", bd)[0] == 7.5
    _kth_check(big, ns // 100, "big ks=1%", bd)
    _kth_check(small, 100, "small")
    assert _kth_check(big, 1, "big ks=1", bd)[0] == 9.25
    _kth_check(small, 255, "small ks=ns")
    assert _kth_check(big, ns, "big ks=ns", bd)[0] == 0.0


# ------------------------------------------------------------------------------------------------
# D. the samplers
SAMPLE_SEEDS = (0, 123, 2 ** 63 + 5)


def _specials(n, seed):
    rng = np.random.default_rng(seed)
    t = rng.standard_normal(n).astype(F32)
    if n > 10:
        t[[3, n - 1]] = np.nan
        t[[5, n // 2]] = -0.0
        t[7] = -np.inf
    return t


def test_dgc_sample_injected_indices():
    """|t[idx]| bit for bit: NaN, -0 (+0 in the sample), duplicates; 300,000 samples is more than
    one trip of the 1,024-workgroup grid."""
    n, ns = 100003, 300000
    t = _specials(n, 1)
    rng = np.random.default_rng(2)
    idx = rng.integers(0, n, ns).astype(np.int64)
    idx[:8] = [3, 5, 7, n - 1, n // 2, 0, 0, n - 1]
    idx[ns - 4:] = [n - 1, 5, 5, 0]
    assert ns > 1024 * K_BLOCK and np.unique(idx).size < ns
    got = ops.dgc_sample(_t(t), ns, sample_idx=_t(idx))
    _same(got, np.abs(t[idx]), "injected sample")
    assert bits(_np(got)[1]) == 0 and np.isnan(_np(got)[0])


@pytest.mark.parametrize("n", [1, 99, 100003, 1 << 24])
def test_dgc_sample_device_generator(n):
    """The device generator's sample is |t[dgc_sample_index(seed, j, n)]| exactly, the same on a
    second call and different under another seed."""
    from tests.device_rng import dgc_sample_index
    t = _specials(n, n)
    td = _t(t)
    ns = max(5000, ns_of(n))
    seen = []
    for seed in SAMPLE_SEEDS:
        idx = dgc_sample_index(seed, np.arange(ns), n)
        assert idx.min() >= 0 and idx.max() < n
        got = ops.dgc_sample(td, ns, seed=seed)
        _same(got, np.abs(t[idx]), f"n={n} seed={seed}")
        _same(ops.dgc_sample(td, ns, seed=seed), _np(got), f"n={n} seed={seed}: second call")
        seen.append(idx)
    if n > 1:
        assert not np.array_equal(seen[0], seen[1]) and not np.array_equal(seen[1], seen[2])


@pytest.mark.parametrize("has_state", [0, 1])
def test_dgc_sample_comp_is_the_sample_of_the_compensated_tensor(has_state):
    n, m = 100003, 0.9
    ns = ns_of(n)
    g, r, a = _specials(n, 31), _specials(n, 32)[::-1].copy(), _specials(n, 33)
    idx = np.random.default_rng(34).integers(0, n, ns).astype(np.int64)
    idx[:6] = [3, 5, 7, n - 1, n - 4, n - 6]
    with np.errstate(invalid="ignore"):
        want_t = O.dgc_memory_compensate(g, r if has_state else None, a if has_state else None, m)[0]
    gd, rd, ad = _t(g), _t(r), _t(a)
    rc, ac = rd.clone(), ad.clone()
    ops.dgc_compensate(gd, rc, ac, has_state, m)
    _same(ac, want_t, "compensated tensor")
    state = (rd, ad) if has_state else (None, None)
    got = ops.dgc_sample_comp(gd, *state, has_state, m, ns, sample_idx=_t(idx))
    _same(got, np.abs(want_t[idx]), "sample_comp, injected, against the oracle")
    _same(got, _np(ops.dgc_sample(ac, ns, sample_idx=_t(idx))), "sample_comp, injected")
    for seed in SAMPLE_SEEDS[1:]:
        got = ops.dgc_sample_comp(gd, *state, has_state, m, ns, seed=seed)
        _same(got, _np(ops.dgc_sample(ac, ns, seed=seed)), f"sample_comp, seed {seed}")
    _same(rd, r, "the residual is only read")
    _same(ad, a, "the accumulator is only read")


# ------------------------------------------------------------------------------------------------
# E. the capacity-bounded record
def test_dgc_capped_record_and_its_mask_update():
    """grace_dgc_write_capped at capacities around the selected count c: header {c, cap, 0, 0},
    the first min(c, cap) entries of the oracle's ascending payload (int32 indices);
    grace_dgc_mask_update_capped multiplies r and a by 0 at exactly those indices."""
    n, ratio = 20000, 0.01
    x, sidx = _random_case(n, 41)
    vals, idx, _, thr = O.dgc_compress(x, sidx, ratio)
    c = int(idx.size)
    assert 3 <= c < n
    rng = np.random.default_rng(42)
    r0, a0 = rng.standard_normal(n).astype(F32), rng.standard_normal(n).astype(F32)
    r0[idx[0]], a0[idx[0]] = np.inf, np.nan              # the first entry travels at every capacity
    r0[idx[1]], a0[idx[1]] = -2.5, -np.inf
    xd = _t(x)
    ws = ops.dgc_threshold_dev(xd, ratio, sample_idx=_t(sidx))
    assert _meta_words(ws) == (bits(thr), c)
    for cap in (1, c - 1, c, c + 1, n):
        rec = ops.dgc_write_capped(xd, ws, cap)
        words = _np(rec)
        assert words.dtype == np.int32 and words.size == ops.exchange_record_words(cap) >= 4 + 2 * cap
        assert words[:4].tolist() == [c, cap, 0, 0], (cap, words[:4])
        m = min(c, cap)
        assert same_bits(words[4:4 + m].view(F32), vals[:m]), cap
        assert np.array_equal(words[4 + cap:4 + cap + m], idx[:m].astype(np.int32)), cap
        r, a = _t(r0), _t(a0)
        ops.dgc_mask_update_capped(rec, cap, r, a)
        er, ea = r0.copy(), a0.copy()
        with np.errstate(invalid="ignore"):
            er[idx[:m]] = r0[idx[:m]] * F32(0)
            ea[idx[:m]] = a0[idx[:m]] * F32(0)
        _same(r, er, f"cap {cap}: r")
        _same(a, ea, f"cap {cap}: a")
        assert np.isnan(er[idx[0]]) and np.isnan(ea[idx[0]])
        if m > 1:
            assert bits(er[idx[1]]) == bits(-0.0) and np.isnan(ea[idx[1]])
