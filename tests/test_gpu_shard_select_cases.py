"""grace_shard_select / grace_shard_clear (csrc/shard.hip) on hand-built records, branch by branch.

The select is a pure function of (records, tab, k, rank, window): every case here builds its records
by hand (tests/shard_select_util.py), asserts through the bookkeeping model that they reach the branch
the case is named after, runs the native select as every rank would (one process plays the ranks,
tests/shard_bf16_util.Ranks) and compares the dense output (canaries on both sides), pay_idx,
sel_gi, the residual (a per-position canary: only the restored positions change, to exactly the
value bits) and the status word BIT FOR BIT with ref_select, the contract of include/grace_hip.h
restated as a numpy sort.  No tolerance: the operation moves values, 0 + v is its only arithmetic;
a bf16 output is that f32 result rounded once (round_cpu: a NaN is 0x7FC0)."""
import numpy as np
import pytest
import torch

from tests import shard_select_util as U
from tests.shard_bf16_util import BF16, CANARY, Ranks

pytestmark = pytest.mark.gpu

F32 = torch.float32
CANARY32 = 0x7FC12345        # f32 output canary: a NaN no select writes here
RES_CANARY = 0x7FD00000      # residual canary at position p: RES_CANARY + p
DTYPES = [pytest.param(F32, id="f32"), pytest.param(BF16, id="bf16")]


def _dev():
    return torch.device("cuda", 0)


def _names(prefix):
    return [n for n in U.CASES if n.startswith(prefix)]


def _ranks_of(world):
    """every rank; above world 8 rank 0, one middle rank and the last"""
    return list(range(world)) if world <= 8 else [0, world // 2, world - 1]


def _out_buffer(dtype, length, off, dev):
    """(the canaried buffer, its zero-filled window [off, off + length) the select writes)"""
    from grace_amd import ops
    if dtype == BF16:
        big = torch.full((length + 8,), CANARY, dtype=torch.int16, device=dev).view(BF16)
        out = big[off:off + length]
        if length:
            ops.fill_bf16(out, 0)
    else:
        big = torch.full((length + 8,), CANARY32, dtype=torch.int32, device=dev).view(F32)
        out = big[off:off + length]
        out.zero_()
    return big, out


def _bits(t):
    """the bit patterns of an f32 / bf16 / int32 tensor as int32 on the CPU"""
    t = t.detach().cpu().contiguous()
    if t.dtype == BF16:
        return t.view(torch.int16).to(torch.int32) & 0xFFFF
    return t.view(torch.int32)


def _res_canary(m, dev):
    return (torch.arange(m, dtype=torch.int32, device=dev) + RES_CANARY).view(F32)


class Case:
    """Hand-built records on the device, and the comparison of one select with the reference."""

    def __init__(self, vals, li, sizes, k, hdr=None):
        self.vals, self.li, self.sizes, self.k = vals, li, list(sizes), k
        self.hdr = list(sizes) if hdr is None else list(hdr)
        self.world, self.cap = vals.shape
        self.bases = U.bases_of(sizes)
        self.n = sum(sizes)
        self.dev = _dev()
        self.R = Ranks(sizes, k, self.dev, cap=self.cap)
        self.R.set_records(vals, li, self.hdr)
        self._sel = {}

    def ref(self, rank, base, length, k=None):
        k = self.k if k is None else k
        r = U.ref_select(self.vals, self.li, self.sizes, self.bases, self.hdr, k, rank, base, length,
                         sel=self._sel.get(k))
        self._sel[k] = r["sel"]
        return r

    def check(self, got, rank, dtype, base, length, off, k=None, sel_gi=True):
        """`got` = (buffer, residual, pay_idx, sel_gi) of one native select against the reference"""
        big, res, pay, sel = got
        ref = self.ref(rank, base, length, k)
        want = U.round_cpu(torch.from_numpy(ref["out_f32"])) if dtype == BF16 else \
            torch.from_numpy(ref["out_f32"]).view(torch.int32)
        can = CANARY if dtype == BF16 else CANARY32
        b = _bits(big)
        assert (b[:off] == can).all() and (b[off + length:] == can).all(), "canaries around the output"
        assert torch.equal(b[off:off + length], want), ("dense output", rank)
        assert np.array_equal(pay.cpu().numpy(), ref["pay_idx"]), ("pay_idx", rank)
        if sel_gi:
            assert np.array_equal(sel.cpu().numpy(), ref["sel_gi"]), ("sel_gi", rank)
        rwant = np.arange(self.sizes[rank], dtype=np.int32) + np.int32(RES_CANARY)
        at, bits = ref["restore"]
        rwant[at] = bits.view(np.int32)
        assert np.array_equal(_bits(res).numpy(), rwant), ("residual", rank)
        return ref

    def run(self, dtype, ranks=None, window=None, off=1, k=None, sel_gi=True, status=None):
        """the native select for `ranks` into canaried buffers, each compared with the reference;
        returns the status bits taken (compared with the reference's unless `status` is given)"""
        from grace_amd import ops
        ranks = _ranks_of(self.world) if ranks is None else ranks
        base, length = (0, self.n) if window is None else window
        bufs = {r: _out_buffer(dtype, length, off, self.dev) for r in ranks}
        res = {r: _res_canary(self.sizes[r], self.dev) for r in ranks}
        rs, pays, sels = self.R.select(res, {r: bufs[r][1] for r in ranks}, out_base={r: base for r in ranks},
                                       k=k, ranks=ranks, sel_gi=sel_gi)
        torch.cuda.synchronize()
        bits = ops.status_take(self.R.status)
        for i, r in enumerate(ranks):
            ref = self.check((bufs[r][0], rs[i], pays[i], sels[i]), r, dtype, base, length, off, k, sel_gi)
        assert bits == (ref["status"] if status is None else status), "status word"
        return bits


def _case(name, k=None):
    """the CASES entry built, model-asserted first; returns (Case, the model)"""
    vals, li, sizes, k0, expect = U.build_case(name)
    k = k0 if k is None else k
    m = U.check_model(name, vals, li, sizes, k, expect)
    return Case(vals, li, sizes, k), m


# ------------------------------------------------------------------ cut population
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", _names("cut-"))
def test_cut_population(name, dtype):
    """T entries share the cut's key bits 31..9: ranked pairwise up to 1024, by the radix select from
    1025; need2 == T takes the whole sub-bin, need2 == 1 and T - 1 split a run of equal keys held
    by different ranks (the lower global index wins)."""
    c, m = _case(name)
    assert m["path"] == ("pairwise" if m["n2"] <= 1024 else "radix")
    assert c.run(dtype) == 0


# ------------------------------------------------------------------ all identical
@pytest.mark.parametrize("name", _names("same-"))
def test_all_entries_identical(name):
    """one bit pattern (1.0, or +0 / -0 mixed) in every slot: the radix select goes through all six
    passes, down to the index digits; at 9 * 4096 + 1 entries ten workgroups fill the cut list"""
    c, m = _case(name)
    assert m["path"] == "radix" and m["index_digits"] and m["n2"] == c.world * c.cap
    assert c.run(F32) == 0


# ------------------------------------------------------------------ k edges
@pytest.mark.parametrize("name", ["k1-two-maxima", "k-valid", "k-valid+1", "cap3000-k10", "w64-cap100-k5000"])
def test_k_edges(name):
    c, m = _case(name)
    assert c.cap != c.k
    bits = c.run(F32)
    assert bits == (2 if name == "k-valid+1" else 0)
    if name == "k1-two-maxima":      # rank 1's maximum (its last slot, global index 15), not rank 2's (34)
        picked = c.ref(0, 0, c.n)["sel_gi"]
        assert picked[picked >= 0].tolist() == [15] and c.bases[1] + int(c.li[1, 2]) == 15
    if name == "k-valid+1":
        assert m["c1"] == -1 and int(c.ref(0, 0, c.n)["sel"].sum()) == m["valid"]


# ------------------------------------------------------------------ special values
@pytest.mark.parametrize("dtype", DTYPES)
def test_special_values_at_every_k(dtype):
    """about 200 patterns (NaNs of several payloads and both signs, +-inf, the largest finite, +-0,
    subnormals, neighbours in the last bit at every bin edge), every k from 1 to valid + 1: the key
    order at every boundary position, NaN above inf, +v / -v and +-0 ties by index"""
    c, m = _case("special", k=1)
    valid = m["valid"]
    assert valid >= 180
    c.run(dtype, k=valid // 2)                    # every rank once
    for k in range(1, valid + 2):
        assert c.run(dtype, ranks=[0], k=k) == (2 if k > valid else 0), k


# ------------------------------------------------------------------ layout
@pytest.mark.parametrize("name", _names("layout-"))
def test_layout(name):
    """partial list blocks, tail pads, a rank with one valid entry, worlds 1 .. 1024"""
    c, m = _case(name)
    if c.world > 1:
        counts = (c.li >= 0).sum(axis=1)
        assert counts.min() == 1 and (counts < c.cap).sum() >= min(2, c.world - 1)
    assert c.run(F32) == 0


def test_large_two_rounds_per_workgroup():
    """world 513 x cap 4096: 513 list blocks on the 512-workgroup grid, so workgroup 0 runs two
    rounds of apply and bnd; every key in C1"""
    c, m = _case("large-w513")
    assert m["rounds"] == 2 and m["grid"] == 512 and int(m["block_counts"].min()) == 4096
    print(f"large: cut sub-bin {m['b2']}, n2 {m['n2']}, need2 {m['need2']}, path {m['path']}")
    assert c.run(F32) == 0


# ------------------------------------------------------------------ windows
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("off", [1, 3])
@pytest.mark.parametrize("kind", ["whole", "inside", "one-selected", "one-rejected"])
def test_windows(kind, off, dtype):
    """the out_base / out_len guard; the window sits at element offsets 1 and 3 of its buffer (2-byte
    alignments for bf16); with and without sel_gi everything else is the same"""
    c, m = _case("window-base")
    ref = c.ref(0, 0, c.n)
    gi = c.bases[2] + c.li[2]
    picked = gi[ref["sel"][2]]
    rejected = gi[(c.li[2] >= 0) & ~ref["sel"][2]]
    assert picked.size and rejected.size
    window = {"whole": None, "inside": (c.n // 4, c.n // 2), "one-selected": (int(picked[0]), 1),
              "one-rejected": (int(rejected[0]), 1)}[kind]
    if window is not None:
        inside = c.ref(0, *window)["out_pos"].size     # selected positions the window holds
        assert (0 < inside < c.k) if kind == "inside" else inside == (1 if kind == "one-selected" else 0)
    for sel_gi in (True, False):
        assert c.run(dtype, window=window, off=off, sel_gi=sel_gi) == 0
    if dtype == BF16:
        assert _out_buffer(dtype, 4, off, c.dev)[1].data_ptr() % 4 == 2


# ------------------------------------------------------------------ status
@pytest.mark.parametrize("which", ["rank0", "last", "mismatch+short"])
def test_status_bits(which):
    """check_records: a header word that differs from tab for rank 0 or for the last rank (bit 1),
    and together with k above the valid entries (bits 1 | 2); every other result is the reference's"""
    vals, li, sizes, k, expect = U.build_case("window-base")
    hdr = list(sizes)
    hdr[0 if which == "rank0" else -1] += 1
    if which == "mismatch+short":
        k = int((li >= 0).sum()) + 1
        assert U.branch_model(vals, li, U.bases_of(sizes), k)["c1"] == -1
    else:
        U.check_model("window-base", vals, li, sizes, k, expect)
    c = Case(vals, li, sizes, k, hdr=hdr)
    assert c.run(F32) == (3 if which == "mismatch+short" else 1)
    assert c.run(BF16, ranks=[1]) == (3 if which == "mismatch+short" else 1)


def _native(fn, c, rank, out, base, pay, sel, res, status_ptr, world=None, cap=None, k=None, ws=None, ws_bytes=None):
    """the C entry point itself (grace_amd/_lib.py), every argument explicit"""
    from grace_amd import _lib, ops
    world = c.world if world is None else world
    cap = c.cap if cap is None else cap
    if ws is None:
        ws = ops.workspace("shardsel", _lib.query("grace_shard_select_workspace_bytes", world, cap), c.dev)
    _lib.call(fn, c.R.recs.data_ptr(), world, rank, cap, c.R.tab.data_ptr(), c.k if k is None else k, res.data_ptr(),
              out.data_ptr(), base, out.numel(), pay.data_ptr(), sel.data_ptr(), ws.data_ptr(),
              ws.numel() if ws_bytes is None else ws_bytes, status_ptr, ops._stream())


@pytest.mark.parametrize("dtype", DTYPES)
def test_null_status_word(dtype):
    """status_host = NULL on records that would set bits 1 and 2: the same results, nothing reported"""
    from grace_amd import ops
    vals, li, sizes, _, _ = U.build_case("window-base")
    hdr = list(sizes)
    hdr[1] -= 1
    c = Case(vals, li, sizes, int((li >= 0).sum()) + 1, hdr=hdr)
    fn = "grace_shard_select" + ("_bf16" if dtype == BF16 else "")
    for rank in range(c.world):
        big, out = _out_buffer(dtype, c.n, 1, c.dev)
        res = _res_canary(c.sizes[rank], c.dev)
        pay = torch.full((c.cap,), -7, dtype=torch.int32, device=c.dev)
        sel = torch.full((c.world * c.cap,), -7, dtype=torch.int32, device=c.dev)
        _native(fn, c, rank, out, 0, pay, sel, res, None)
        torch.cuda.synchronize()
        assert c.check((big, res, pay, sel), rank, dtype, 0, c.n, 1)["status"] == 3
    assert ops.status_take(c.R.status) == 0
    assert c.run(dtype) == 3                      # and with the word, the bits arrive


# ------------------------------------------------------------------ history on one workspace
HIST_BYTES = 2 * U.GROUPS * U.BINS * 4


def test_history_leaves_the_workspace_zeroed():
    """one sequence on the shared workspace: radix ties, the c1 = -1 path, 4097 entries, ten list
    blocks, a header mismatch, the first again.  After every call the result is the reference's and
    the two histogram areas and the ctl counters n2 and ticket read zero (`need` is rewritten by
    every call)."""
    from grace_amd import _lib, ops
    dev = _dev()
    names = ["same-one-n4096-k2048", "k-valid+1", "layout-w1-n4097", "layout-w5-n9x4096+1", "window-base",
             "same-one-n4096-k2048"]
    cases = {n: _case(n)[0] for n in set(names)}
    hdr = list(cases["window-base"].sizes)
    hdr[0] += 3
    cases["window-base"] = Case(cases["window-base"].vals, cases["window-base"].li, cases["window-base"].sizes,
                                cases["window-base"].k, hdr=hdr)
    need = max(int(_lib.query("grace_shard_select_workspace_bytes", c.world, c.cap)) for c in cases.values())
    ws = ops.workspace("shardsel", need, dev)      # one buffer for the whole sequence
    for step, name in enumerate(names):
        c = cases[name]
        for dtype in (F32, BF16):
            bits = c.run(dtype, ranks=[0, c.world - 1] if c.world > 1 else [0])
            assert bits == {"k-valid+1": 2, "window-base": 1}.get(name, 0), (step, name)
            assert ops.workspace("shardsel", need, dev).data_ptr() == ws.data_ptr()
            head = ws[:256 + HIST_BYTES].cpu().numpy()
            ctl = head[:64].view(np.uint32)
            assert ctl[3] == 0 and ctl[4] == 0, (step, name, "n2 / ticket")
            assert not head[256:].any(), (step, name, "histogram copies")


# ------------------------------------------------------------------ host refusals
@pytest.mark.parametrize("dtype", DTYPES)
def test_refusals_leave_the_outputs_untouched_and_go_on(dtype):
    from grace_amd import _lib
    c, _ = _case("k1-two-maxima")
    fn = "grace_shard_select" + ("_bf16" if dtype == BF16 else "")
    exact = int(_lib.query("grace_shard_select_workspace_bytes", c.world, c.cap))
    small = torch.zeros(4096, dtype=torch.uint8, device=c.dev)
    refused = [
        ("world 1025", dict(world=1025, ws=small), "bad arguments"),
        ("rank = world", dict(rank=c.world), "bad arguments"),
        ("cap 0", dict(cap=0, ws=small), "bad arguments"),
        ("k 0", dict(k=0), "bad arguments"),
        ("world * cap = 2^31", dict(world=1024, cap=1 << 21, ws=small), "bad arguments"),   # the argument check first
        ("workspace one byte short", dict(ws_bytes=exact - 1), "workspace too small"),
    ]
    for what, kw, msg in refused:
        big, out = _out_buffer(dtype, c.n, 1, c.dev)
        out.view(torch.int16 if dtype == BF16 else torch.int32).fill_(CANARY if dtype == BF16 else CANARY32)
        res = _res_canary(c.sizes[0], c.dev)
        pay = torch.full((c.cap,), -7, dtype=torch.int32, device=c.dev)
        sel = torch.full((c.world * c.cap,), -7, dtype=torch.int32, device=c.dev)
        kw = dict(kw)
        rank = kw.pop("rank", 0)
        with pytest.raises(_lib.GraceNativeError, match=f"{fn}: {msg}"):
            _native(fn, c, rank, out, 0, pay, sel, res, c.R.status.data_ptr(), **kw)
        torch.cuda.synchronize()
        assert (_bits(big) == (CANARY if dtype == BF16 else CANARY32)).all(), what
        assert (pay == -7).all() and (sel == -7).all(), what
        assert torch.equal(_bits(res), _bits(_res_canary(c.sizes[0], c.dev))), what
        assert c.run(dtype) == 0, what             # a good call afterwards is right


# ------------------------------------------------------------------ the clear
CLEAR_COUNTS = [0, 1, 2047, 2048, 2049, 1024 * 2048 + 2049]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("count", CLEAR_COUNTS)
def test_shard_clear_counts(count, dtype):
    """grace_shard_clear at its 2048-entry round edges and past its 1024-workgroup grid: the list
    holds -1, positions on both sides of the window and repeated positions"""
    from grace_amd import _lib, ops
    dev = _dev()
    base, off = 1000, 1
    length = max(5000, (count * 3) // 2)
    rng = np.random.default_rng(count)
    gi = rng.integers(-1, base + length + 1000, max(count, 1)).astype(np.int32)
    gi[::5] = gi[0]
    gi[1::7] = -1
    if count >= 2047:
        gi[[2, 3, count - 1]] = [base, base + length - 1, base + length]      # the window's ends, and one past
        assert (gi < base).sum() > 100 and (gi >= base + length).sum() > 100 and (gi == -1).sum() > 100
    filled = 0x40E0 if dtype == BF16 else 0x40E00000                           # 7.0
    can = CANARY if dtype == BF16 else CANARY32
    big = torch.full((length + 8,), can, dtype=torch.int16 if dtype == BF16 else torch.int32, device=dev)
    big[off:off + length] = filled
    out = big.view(dtype)[off:off + length]
    sel = torch.from_numpy(gi).to(dev)
    if count == 0:      # an empty tensor has no address: the entry point itself, a valid pointer and count 0
        _lib.call("grace_shard_clear" + ("_bf16" if dtype == BF16 else ""), out.data_ptr(), base, length,
                  sel.data_ptr(), 0, ops._stream())
    else:
        assert ops.shard_clear(out, base, sel[:count]) is out
    torch.cuda.synchronize()
    want = np.full(length + 8, can, dtype=np.int32)
    want[off:off + length] = filled
    g = gi[:count].astype(np.int64)
    want[off + g[(g >= base) & (g < base + length)] - base] = 0
    assert np.array_equal(_bits(big.view(dtype)).numpy(), want)
    if count >= 2047:
        assert (want[off:off + length] == 0).sum() > 100 and (want[off:off + length] == filled).sum() > 100
