"""The sharded top-k step on bfloat16 shards with a bfloat16 dense result, NATIVE kernels
(grace_amd/sharded_bf16.py; grace_shard_select_bf16, grace_shard_clear_bf16, grace_fill_bf16).

For a bf16 shard every result is what the f32 sharded step gives for ``shard.float()``: payloads,
residuals, pay_idx and sel_gi bit for bit, and the dense result == the f32 step's rounded once to
nearest even (``out_f32.to(torch.bfloat16)``, converted on the CPU), a NaN becoming 0x7FC0.  The
select is exercised at every site that stores a selected value (shard_take's four callers), the
rounding at its edges, the window and 2-byte alignments of `out`, the clear and the fill against
canaries, and the class at world 1 and at world 3 (three processes on one GPU over gloo) against
the parent class and the oracle (TopKCompressor, grace_dl/dist/compressor/topk.py:32-42;
ResidualMemory, memory/residual.py:10-20)."""
import os
import tempfile

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from oracle import grace_oracle as O
from tests.golden_util import same_bits
from tests.shard_bf16_util import BF16, CANARY, Ranks, bits16, from_bits16, same_i32
from tests.shard_select_util import round_cpu as _round_cpu
from tests.test_sharded_bf16_gloo import _bucket as bf16_bucket
from tests.test_sharded_bf16_gloo import _check_step

pytestmark = pytest.mark.gpu


def _dev():
    return torch.device("cuda", 0)


def _normals(case, n, seed):
    rng = np.random.default_rng(seed)
    g = rng.standard_normal(n).astype(np.float32)
    if case == "ties":
        g[rng.random(n) < 0.7] = 0.0
    return g


def _sizes(n, world):
    return [n // world + (1 if r < n % world else 0) for r in range(world)]


def _zeros16(n, dev):
    from grace_amd import ops
    return ops.fill_bf16(torch.empty(n, dtype=BF16, device=dev), 0)


# ------------------------------------------------------------------ 1. the select, every store site
@pytest.mark.parametrize("world,n,case,ratio", [
    (5, 50001, "normal", 0.01),       # 2,500 entries: one partial block
    (3, 3000001, "ties", 0.4),        # the cut among ~2.1 M zeros: the last arriver's radix select
    (4, 1 << 23, "normal", 0.1),      # 3.36 M entries > 512 * 4096: several rounds per workgroup
])
def test_select_bf16_equals_the_f32_select_rounded_once(world, n, case, ratio):
    from grace_amd import ops
    dev = _dev()
    k = O.ratio_k(n, ratio)
    R = Ranks(_sizes(n, world), k, dev)
    g = _normals(case, n, 77 + world)      # full-precision f32: the selected values have low bits
    res = R.local(torch.from_numpy(g).to(dev))
    out32 = [torch.zeros(n, device=dev) for _ in range(world)]
    r32, p32, s32 = R.select(res, out32)
    out16 = [_zeros16(n, dev) for _ in range(world)]
    r16, p16, s16 = R.select(res, out16)
    torch.cuda.synchronize()
    assert ops.status_take(R.status) == 0
    for r in range(world):
        assert same_i32(r16[r], r32[r]) and torch.equal(p16[r], p32[r]) and torch.equal(s16[r], s32[r])
        assert torch.equal(out16[r].view(torch.int16), out16[0].view(torch.int16))
        assert same_i32(out32[r], out32[0])
    assert int((s32[0] >= 0).sum()) == k
    low = int(((out32[0].view(torch.int32) & 0xFFFF) != 0).sum())
    print(f"selected {k}, with non-zero low 16 bits {low}")
    assert 2 * low >= k                    # the rounding is exercised, not the identity
    got = bits16(out16[0])
    assert torch.equal(got, _round_cpu(out32[0]))
    if n == 50001:
        _, _, i_or, r_or, out_or = O.topk_residual_step(g, None, ratio)
        assert torch.equal(got, _round_cpu(torch.from_numpy(out_or)))
        assert same_bits(np.concatenate([x.cpu().numpy() for x in r16]), r_or)
        idx = np.concatenate([p.cpu().numpy() for p in p16]).astype(np.int64)
        assert np.array_equal(np.sort(idx[idx >= 0]), np.sort(i_or.astype(np.int64)))


# ------------------------------------------------------------------ 2. rounding edges through the select
UPPER = [0x0000, 0x8000, 0x0001, 0x8001, 0x007F, 0x0080, 0x3F80, 0xBF80, 0x3FFF, 0x4049, 0x7F7F, 0xFF7F,
         0x7F80, 0xFF80, 0x7FC0, 0xFFC1]     # +-0, subnormals, 1, 0x7F7F (rounds up to inf), +-inf, NaNs
LOWER = [0x0000, 0x0001, 0x7FFF, 0x8000, 0x8001, 0xFFFF]


@pytest.mark.parametrize("k_of", ["all", "all+1", "half"])
def test_select_bf16_rounding_edges(k_of):
    """Hand-made records at W = 2, cap = 2048: 16 upper halves x the six lower halves that decide a
    rounding.  The stored value is 0 + v (the f32 select's own arithmetic, so -0 is written as +0),
    rounded once: compared with the CPU's conversion (_round_cpu: a NaN is 0x7FC0) and with the f32
    select, no exception list.
    k = all valid entries selects everything through the coarse cut; one more than that is the
    c1 = -1 path (every valid entry selected, status bit 2: fewer valid entries than k)."""
    from grace_amd import ops
    dev = _dev()
    bits = np.array([(u << 16) | lo for u in UPPER for lo in LOWER], dtype=np.uint32)
    vals = bits.view(np.float32)
    nv = vals.size
    assert nv == 96
    k = {"all": nv, "all+1": nv + 1, "half": nv // 2}[k_of]
    R = Ranks([3000, 3000], k, dev, cap=2048)
    li = [7 * np.arange(48) + 1, 5 * np.arange(48) + 2]
    for r in range(2):
        v, i = R.slot(r)
        v[:48] = torch.from_numpy(vals[48 * r:48 * r + 48].copy()).to(dev)
        i[:48] = torch.from_numpy(li[r].astype(np.int32)).to(dev)
    res = [torch.zeros(3000, device=dev) for _ in range(2)]
    out32 = [torch.zeros(R.n, device=dev) for _ in range(2)]
    r32, p32, s32 = R.select(res, out32)
    out16 = [_zeros16(R.n, dev) for _ in range(2)]
    r16, p16, s16 = R.select(res, out16)
    torch.cuda.synchronize()
    assert ops.status_take(R.status) == (2 if k_of == "all+1" else 0)
    for r in range(2):
        assert same_i32(r16[r], r32[r]) and torch.equal(p16[r], p32[r]) and torch.equal(s16[r], s32[r])
        assert torch.equal(bits16(out16[r]), _round_cpu(out32[r]))
    sel = s16[0].cpu().numpy().reshape(2, 2048)
    assert (sel[:, 48:] == -1).all()
    picked = sel[:, :48] >= 0
    assert int(picked.sum()) == min(k, nv)
    gi = np.stack([li[0], li[1] + 3000])
    assert np.array_equal(sel[:, :48][picked], gi[picked])
    # the written positions against the CPU's rounding of 0 + v
    want = np.zeros(R.n, np.float32)
    with np.errstate(invalid="ignore"):
        want[gi[picked]] = np.float32(0.0) + vals.reshape(2, 48)[picked]
    assert torch.equal(bits16(out16[0]), _round_cpu(torch.from_numpy(want)))
    assert int((bits16(out16[0]) == 0x7FC0).sum()) == 22     # every NaN (the largest keys: selected at any k here)


# ------------------------------------------------------------------ 3. / 4. windows, alignment, the clear
WIN_BASE, WIN_LEN = 70001, 9001


@pytest.fixture(scope="module")
def windowed():
    """One bucket of 100003 elements over 3 ranks, k = 5000 (15000 gathered entries: not a multiple of
    2048, two thirds of sel_gi are -1), its f32 select on the whole range, computed once."""
    dev = _dev()
    n = 100003
    R = Ranks(_sizes(n, 3), 5000, dev)
    res = R.local(torch.from_numpy(_normals("normal", n, 5)).to(dev))
    out32 = [torch.zeros(n, device=dev) for _ in range(3)]
    r32, p32, s32 = R.select(res, out32)
    torch.cuda.synchronize()
    return {"R": R, "res": res, "r32": r32, "p32": p32, "s32": s32, "ref": _round_cpu(out32[0])}


@pytest.mark.parametrize("off", [1, 3])
def test_select_bf16_window_at_2_byte_alignment(windowed, off):
    from grace_amd import ops
    W, dev = windowed, _dev()
    R = W["R"]
    bigs = [from_bits16([CANARY] * (WIN_LEN + 8), dev) for _ in range(3)]
    outs = [b[off:off + WIN_LEN] for b in bigs]
    for o in outs:
        assert o.data_ptr() % 16 == 2 * off
        ops.fill_bf16(o, 0)
    r16, p16, s16 = R.select(W["res"], outs, out_base=[WIN_BASE] * 3)
    torch.cuda.synchronize()
    assert ops.status_take(R.status) == 0
    ref = W["ref"][WIN_BASE:WIN_BASE + WIN_LEN]
    assert int((ref != 0).sum()) > 100
    for r in range(3):
        b = bits16(bigs[r])
        assert (b[:off] == CANARY).all() and (b[off + WIN_LEN:] == CANARY).all()
        assert torch.equal(b[off:off + WIN_LEN], ref)
        assert same_i32(r16[r], W["r32"][r]) and torch.equal(p16[r], W["p32"][r]) and torch.equal(s16[r], W["s32"][r])


@pytest.mark.parametrize("off,base,length", [(1, 0, 100003), (3, WIN_BASE, WIN_LEN), (2, 33335, 1)])
def test_shard_clear_bf16(windowed, off, base, length):
    from grace_amd import ops
    dev = _dev()
    sel = windowed["s32"][0]
    assert sel.numel() % 2048 != 0 and int((sel == -1).sum()) == 10000
    big = from_bits16([CANARY] * (length + 8), dev)
    ops.shard_clear(big[off:off + length], base, sel)
    torch.cuda.synchronize()
    gi = sel.cpu().numpy().astype(np.int64)
    gi = gi[(gi >= base) & (gi < base + length)] - base
    want = np.full(length + 8, CANARY, dtype=np.int32)
    want[off + gi] = 0
    assert torch.equal(bits16(big), torch.from_numpy(want))
    # the f32 clear through the dispatch is the one it was
    big32 = torch.full((length + 8,), 7.0, device=dev)
    ops.shard_clear(big32[off:off + length], base, sel)
    want32 = np.full(length + 8, 7.0, dtype=np.float32)
    want32[off + gi] = 0.0
    assert same_bits(big32.cpu().numpy(), want32)


# ------------------------------------------------------------------ 5. the fill
@pytest.mark.parametrize("bits", [0, 0x3F80])
def test_fill_bf16(bits):
    from grace_amd import ops
    dev = _dev()
    for length in (0, 1, 7, 8, 9, 4097, (1 << 20) + 3):
        for off in range(8):
            big = torch.full((length + 16,), CANARY, dtype=torch.int16, device=dev)
            x = big.view(BF16)[off:off + length]
            assert ops.fill_bf16(x, bits) is x
            want = torch.full((length + 16,), CANARY, dtype=torch.int16, device=dev)
            want[off:off + length] = bits
            assert torch.equal(big, want), (length, off)


# ------------------------------------------------------------------ 6. the class at world 1
def _bf16_normals(m, seed, dev):
    return bf16_bucket(m, seed)[0].to(dev)


def _step_equal(eng, ref, want32, out, name="b"):
    """`out` of the engine under test against the f32 engine's result `want32` of the same step"""
    if out.dtype == BF16:
        assert torch.equal(bits16(out), _round_cpu(want32))
    else:
        assert out.dtype == torch.float32 and same_i32(out, want32)
    assert same_i32(eng.residuals[name], ref.residuals[name])
    # the payload as a set (the order of a record's entries is the local pass's arrival order)
    (va, ia), (vb, ib) = eng.last_payload, ref.last_payload
    oa, ob = torch.argsort(ia), torch.argsort(ib)
    assert int((ia >= 0).sum()) > 0 and torch.equal(ia[oa], ib[ob])
    keep = ia[oa] >= 0
    assert same_i32(va[oa][keep].contiguous(), vb[ob][keep].contiguous())


@pytest.mark.parametrize("m", [40003, 9001])     # the multi-workgroup local pass / below TOPK_SMALL_N
def test_class_world1_against_the_f32_class(m):
    from grace_amd.dist.sharded import ShardedTopK as F32ShardedTopK
    from grace_amd.sharded_bf16 import ShardedTopK
    dev = _dev()
    steps = 3
    eng, ref, fresh = ShardedTopK(0.01), F32ShardedTopK(0.01), ShardedTopK(0.01, recycle_output=False)
    changed = 0
    for s in range(steps):
        g = _bf16_normals(m, 40 + s, dev)
        out = eng.step(g, "b")
        want = ref.step(g.float(), "b")
        assert out.dtype == BF16 and out.shape == (m,)
        _step_equal(eng, ref, want, out)
        # a recycled output equals a fresh one
        assert torch.equal(bits16(out), bits16(fresh.step(g, "b")))
        if s >= 1:
            changed += int((out.float() != want).sum())
        del out, want         # dropped: the next step takes it back
    assert changed > 0        # from step 1 on t = r + g has low bits
    assert eng._recycler_bf16.hits == steps - 1 and eng._recycler.hits == 0
    assert fresh._recycler_bf16.hits == 0
    eng.check()
    fresh.check()


def test_class_held_result_is_not_recycled():
    from grace_amd.sharded_bf16 import ShardedTopK
    dev = _dev()
    eng = ShardedTopK(0.01)
    held = eng.step(_bf16_normals(40003, 1, dev), "b")
    snap = bits16(held)
    out = eng.step(_bf16_normals(40003, 2, dev), "b")
    torch.cuda.synchronize()
    assert out.data_ptr() != held.data_ptr() and eng._recycler_bf16.hits == 0
    assert torch.equal(bits16(held), snap)
    eng.check()


def test_class_dtype_switch_keeps_the_residual_and_the_outputs_apart():
    """bf16, f32, bf16, f32, bf16 on one name, every result dropped: the residual is the all-f32
    run's, every result has its shard's dtype, and each dtype recycles its own previous output
    through its own selection list (a list shared with the other dtype's step in between would
    leave stale values behind)."""
    from grace_amd.dist.sharded import ShardedTopK as F32ShardedTopK
    from grace_amd.sharded_bf16 import ShardedTopK
    dev = _dev()
    eng, ref = ShardedTopK(0.01), F32ShardedTopK(0.01)
    for s, dtype in enumerate([BF16, torch.float32, BF16, torch.float32, BF16]):
        g = _bf16_normals(40003, 60 + s, dev)
        out = eng.step(g if dtype == BF16 else g.float(), "b")
        want = ref.step(g.float(), "b")
        assert out.dtype == dtype
        _step_equal(eng, ref, want, out)
        del out, want
    assert eng._recycler_bf16.hits == 2 and eng._recycler.hits == 1
    eng.check()


def test_class_f32_shard_is_the_parent_path_and_float16_raises():
    from grace_amd.dist.sharded import ShardedTopK as F32ShardedTopK
    from grace_amd.sharded_bf16 import ShardedTopK
    dev = _dev()
    eng, ref = ShardedTopK(0.01), F32ShardedTopK(0.01)
    for s in range(2):
        g = torch.from_numpy(_normals("normal", 40003, 80 + s)).to(dev)
        out, want = eng.step(g, "b"), ref.step(g.clone(), "b")
        assert out.dtype == torch.float32
        _step_equal(eng, ref, want, out)
        del out, want
    assert eng._recycler.hits == 1 and eng._recycler_bf16.hits == 0
    with pytest.raises(TypeError):
        eng.step(torch.zeros(1000, dtype=torch.float16, device=dev), "h")
    eng.check()


# ------------------------------------------------------------------ 7. world 3 over gloo, one GPU
W3_SIZES = [70001, 9001, 40002]
W3_STEPS = 3


def _w3_worker(rank, world, path, outdir):
    dist.init_process_group("gloo", init_method=f"file://{path}", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    from grace_amd.sharded_bf16 import ShardedTopK
    n, base, m = sum(W3_SIZES), sum(W3_SIZES[:rank]), W3_SIZES[rank]
    res = {}
    for dense in ("replicated", "shard"):
        eng = ShardedTopK(0.01, dense=dense)
        tag = f"0.01_{dense}_"
        for s in range(W3_STEPS):
            # the shard is a slice at element offset 1 of a larger tensor: g is only 2-byte aligned
            big = torch.empty(m + 1, dtype=BF16, device="cuda")
            big[1:] = bf16_bucket(n, 100 + s)[0][base:base + m]
            assert big[1:].data_ptr() % 4 == 2
            # the result is dropped right away: the next step recycles it
            o = eng.step(big[1:], "bucket")
            assert o.dtype == BF16
            res[tag + f"out{s}"] = o.view(torch.int16).cpu().numpy()
            del o
            v, i = eng.last_payload
            v, i = v.cpu().numpy(), i.cpu().numpy()
            res[tag + f"vals{s}"] = v[i >= 0]
            res[tag + f"idx{s}"] = i[i >= 0]
            res[tag + f"res{s}"] = eng.residuals["bucket"].cpu().numpy()
        eng.check()
        res[tag + "host_reads"] = np.array([eng.host_reads])
        res[tag + "recycled"] = np.array([eng._recycler_bf16.hits])
    np.savez(os.path.join(outdir, f"r{rank}.npz"), **res)
    dist.destroy_process_group()


def test_class_world3_matches_the_oracle():
    world = 3
    with tempfile.TemporaryDirectory() as tmp:
        mp.spawn(_w3_worker, args=(world, os.path.join(tmp, "rdv"), tmp), nprocs=world, join=True)
        outs = []
        for r in range(world):
            with np.load(os.path.join(tmp, f"r{r}.npz")) as z:
                outs.append({k: z[k] for k in z.files})
    n = sum(W3_SIZES)
    steps = []
    r = None
    for s in range(W3_STEPS):      # the oracle on the widened bucket, once for both modes
        _, v, i, r, out = O.topk_residual_step(bf16_bucket(n, 100 + s)[1], r, 0.01)
        steps.append((v, i, r, out))
    for dense in ("replicated", "shard"):
        tag = f"0.01_{dense}_"
        for s, (v, i, r, out) in enumerate(steps):
            _check_step(outs, tag, s, W3_SIZES, v, i, r, out, dense)
        assert all(int(o[tag + "host_reads"][0]) == 1 for o in outs)
        assert all(int(o[tag + "recycled"][0]) == W3_STEPS - 1 for o in outs)
