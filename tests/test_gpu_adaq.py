"""Adaptive quantisation (grace_amd/csrc/adaq.hip) against a numpy restatement of
include/grace_hip_adaq.h: a stable argsort on (-|x|, index) per class, math.fsum for the means, payloads
built byte by byte.  Everything but the two means is compared bit for bit.  The means: the device adds at
most k <= 2^22 same-sign f64 numbers and the ties' product, each rounding at most 2^-53 of the final sum,
so its f64 mean is within 2^-31 of the exact one and its f32 rounding within 1 ulp of fsum's."""
import datetime
import functools
import math
import os
import tempfile
import time

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from grace_amd import _lib, ops
from grace_amd.adaq import AdaqCompressor, grace_from_params
from grace_amd.dist.communicator.allgather import Allgather
from grace_amd.dist.memory.none import NoneMemory
from grace_amd.dist.memory.residual import ResidualMemory

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
f32, C = np.float32, 8192
DTYPES = pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
# adaq.hip: count, place and decode launch one workgroup a chunk, uncapped; only the histogram passes' grid
# stops, at 512 workgroups of 1024 threads and 16 B a thread, so one sweep of them is 2^21 f32 or 2^22 bf16
# elements and N_SWEEP is past it
N_ODD, N_SWEEP, N_TIES = 3 * C + 5, (1 << 22) + 4099, 2 * C + 3


def bits(t):
    t = t.detach().cpu().contiguous().reshape(-1)
    return t.view(torch.int16 if t.dtype == BF16 else torch.int32).numpy()


def on_device(x, dtype):
    """(device tensor of x in dtype, its values widened to f32 numpy)"""
    t = torch.from_numpy(np.asarray(x, f32)).to(dtype)
    return t.to(DEV), t.float().numpy()


@functools.lru_cache(None)
def spread(n, dtype, seed=0):
    """n + 1 elements with magnitudes over 2^-30 .. 2^3, both signs, about 10 % zeros of either sign"""
    rng = np.random.default_rng(n + seed)
    x = rng.choice([-1.0, 1.0], n + 1) * (1 + rng.random(n + 1)) * 2.0 ** rng.integers(-30, 3, n + 1)
    return on_device(x * (rng.random(n + 1) >= 0.1), dtype)


def ref_select(x, ratio):
    """the header's selection: (selected, negative, the two fsum means as f32)"""
    u = x.view(np.uint32)
    mag, neg = (u & 0x7FFFFFFF).astype(np.int64), (u >> 31).astype(bool)
    sel, means = np.zeros(x.size, bool), []
    for cls in (~neg & (mag != 0), neg & (mag != 0)):
        idx = np.flatnonzero(cls)
        k = math.ceil(float(idx.size) * ratio) if idx.size else 0
        take = idx[np.argsort(-mag[idx], kind="stable")[:k]]
        sel[take] = True
        means.append(f32(math.fsum(x[take].astype(np.float64).tolist()) / k) if k else f32(0))
    return sel, neg, means


def ref_decode(sel, neg, means):
    return np.where(sel, np.where(neg, f32(means[1]), f32(means[0])), f32(0)).astype(f32)


def ref_payload(n, cap, sel, neg, means):
    pos = np.flatnonzero(sel)
    nch = -(-n // C)
    ends = np.searchsorted(pos, np.arange(1, nch + 1) * C).astype(np.uint32)
    ent = (neg[pos].astype(np.uint16) << 15 | (pos % C).astype(np.uint16)).tobytes() + bytes(2 * (cap - pos.size))
    return b"".join([np.array(means, f32).tobytes(), np.array([pos.size, cap], np.uint32).tobytes(),
                     ends.tobytes(), bytes(-4 * nch % 16), ent, bytes(-len(ent) % 16)])


def ulps(a, b):
    a, b = (np.array(v, f32).view(np.int32).astype(np.int64) for v in (a, b))
    return np.abs(a - b).max()


def check(xd, x, ratio):
    n = x.size
    cap = ops.adaq_capacity(n, ratio)
    assert cap == math.ceil(float(n) * ratio) + 4 == _lib.query("grace_adaq_capacity", n, float(ratio))
    pay = ops.adaq_compress(xd, ratio)
    raw = pay.cpu().numpy().tobytes()
    assert len(raw) == ops.adaq_payload_bytes(n, ratio) == _lib.query("grace_adaq_payload_bytes", n, float(ratio))
    sel, neg, means = ref_select(x, ratio)
    got = np.frombuffer(raw[:8], f32)
    assert sel.sum() <= cap and raw[8:] == ref_payload(n, cap, sel, neg, got)[8:]
    assert np.array_equal(got, means) if not np.isfinite(means).all() else ulps(got, means) <= 1, (got, means)
    assert ops.adaq_compress(xd, ratio).cpu().numpy().tobytes() == raw
    want = bits(torch.from_numpy(ref_decode(sel, neg, got)).to(xd.dtype))
    dec = ops.adaq_decode_aggregate(pay, 1, n, ratio, out_dtype=xd.dtype)
    step = ops.adaq_step_w1(xd, ratio)
    assert dec.dtype == step.dtype == xd.dtype and step.shape == xd.shape
    assert np.array_equal(bits(dec), want) and np.array_equal(bits(step), want)
    return sel, got


@pytest.mark.parametrize("ratio", [0.01, 0.3, 1.0])
@DTYPES
@pytest.mark.parametrize("n", [1, C - 1, C, C + 1, N_ODD, N_SWEEP])
def test_encode_at_every_size(n, dtype, ratio):
    xd, x = spread(n, dtype)
    check(xd[:n], x[:n], ratio)


def tie_cases(rng):
    sp = np.array(spread(N_TIES, F32)[1][:N_TIES])
    inf = sp.copy()
    inf[rng.choice(N_TIES, 8, replace=False)] = [np.inf] * 5 + [-np.inf] * 3
    return {"all_equal": np.full(N_TIES, 1.5), "all_zero": np.resize([0.0, -0.0], N_TIES), "all_positive": np.abs(sp),
            "few_values": rng.choice([1.0, -1.0, 2.0, -2.0, 0.0], N_TIES), "inf": inf, "denormal": sp * 2.0 ** -120}


@DTYPES
@pytest.mark.parametrize("case", ["all_equal", "all_zero", "all_positive", "few_values", "inf", "denormal"])
def test_ties_and_empty_classes(case, dtype):
    xd, x = on_device(tie_cases(np.random.default_rng(7))[case], dtype)
    sel, means = check(xd, x, 0.3)
    if case == "all_equal":       # the lowest k indices
        assert np.array_equal(np.flatnonzero(sel), np.arange(math.ceil(N_TIES * 0.3)))
    if case == "all_zero":
        assert not sel.any() and np.array_equal(means.view(np.uint32), [0, 0])
    if case == "few_values":      # both cuts fall inside the runs of +2 and -2, which span the chunks
        assert all(0 < sel[x == v].sum() < (x == v).sum() for v in (2, -2)) and not sel[np.abs(x) == 1].any()


@DTYPES
def test_gradient_off_the_vector_grid(dtype):
    """the gradient one element past a 16-byte boundary"""
    xd, x = spread(N_ODD, dtype)
    assert xd.data_ptr() % 16 == 0
    check(xd[1:], x[1:], 0.3)


def rank_payloads(world, n):
    """hand-written payloads, each rank with its own entries and means: (selected, negative, means) a rank"""
    rng = np.random.default_rng(world)
    return [(rng.random(n) < 0.05, rng.random(n) < 0.5, rng.standard_normal(2).astype(f32)) for _ in range(world)]


def rank_sum(ds, divisor, out_dtype):
    acc = np.zeros(ds[0].size, f32)
    for d in ds:
        acc = acc + d
    return bits(torch.from_numpy(acc / f32(divisor) if divisor != 1 else acc).to(out_dtype))


@pytest.mark.parametrize("out_dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("divisor", [1, 3])
@pytest.mark.parametrize("world", [3, 65])
def test_decode_across_ranks(world, divisor, out_dtype):
    n, ratio = 2 * C + 5, 0.1
    cap = ops.adaq_capacity(n, ratio)
    ranks = rank_payloads(world, n)
    wire = np.frombuffer(b"".join(ref_payload(n, cap, *r) for r in ranks), np.uint8)
    got = ops.adaq_decode_aggregate(torch.from_numpy(wire.copy()).to(DEV), world, n, ratio, divisor=divisor,
                                    out_dtype=out_dtype)
    assert got.dtype == out_dtype and np.array_equal(bits(got), rank_sum([ref_decode(*r) for r in ranks], divisor, out_dtype))


def test_decoder_refusals():
    """rank 0's header cap differs: zeros; rank 1's last chunk has `ends` stepping backwards: that chunk is
    zeros; rank 2 has an entry past the ragged end of the last chunk: it is skipped.  The rest decodes."""
    n, ratio = 2 * C + 5, 0.1
    cap = ops.adaq_capacity(n, ratio)
    ranks = rank_payloads(4, n)
    ranks[1][0][-2] = ranks[2][0][-1] = True                  # entries in the ragged chunk; rank 2's is its last
    pays = [np.frombuffer(ref_payload(n, cap, *r), np.uint8).copy() for r in ranks]
    ds = [ref_decode(*r) for r in ranks]
    pays[0].view(np.uint32)[3] = cap + 1
    ds[0][:] = 0
    pays[1].view(np.uint32)[4 + 2] = pays[1].view(np.uint32)[4 + 1] - 1
    ds[1][2 * C:] = 0
    last = 16 + 16 + 2 * (int(ranks[2][0].sum()) - 1)
    pays[2][last:last + 2].view(np.uint16)[0] = (pays[2][last:last + 2].view(np.uint16)[0] & 0x8000) | 100
    ds[2][-1] = 0
    got = ops.adaq_decode_aggregate(torch.from_numpy(np.concatenate(pays)).to(DEV), 4, n, ratio)
    assert all(d.any() for d in ds[1:]) and np.array_equal(bits(got), rank_sum(ds, 1, F32))


@DTYPES
def test_classes_at_world1(dtype):
    xd, x = spread(N_ODD, dtype)
    xd, x = xd[:3 * 4099].view(3, 4099), x[:3 * 4099]
    sel, neg, _ = ref_select(x, 0.05)
    means = np.frombuffer(ops.adaq_compress(xd, 0.05)[:8].cpu().numpy().tobytes(), f32)
    want = bits(torch.from_numpy(ref_decode(sel, neg, means)).to(dtype))
    for comm in (Allgather(AdaqCompressor(0.05), NoneMemory(), 1),
                 grace_from_params({'compressor': 'adaq', 'memory': 'none', 'communicator': 'allgather',
                                    'world_size': 1, 'compress_ratio': 0.05})):
        out = comm.step(xd, "w")
        assert out.dtype == dtype and out.shape == xd.shape and np.array_equal(bits(out), want)
    if dtype == F32:              # the unfused path: error feedback leaves residual = t - decode
        comm = Allgather(AdaqCompressor(0.05), ResidualMemory(), 1)
        out = comm.step(xd, "w")
        assert out.shape == xd.shape and np.array_equal(bits(out), want)
        assert np.array_equal(bits(comm.memory.residuals["w"]), (x - ref_decode(sel, neg, means)).view(np.int32))


def test_decode_aggregate_gathered_equals_the_decompress_loop():
    comp = AdaqCompressor(0.1)
    pay = [comp.compress(spread(4099, F32, seed=s)[0][:4099] * 2.0 ** -s, "w") for s in (0, 5)]
    got = comp.decode_aggregate_gathered([torch.cat([p[0][0] for p in pay])], pay[0][1], 2)
    want = np.zeros(4099, f32)
    for p, ctx in pay:
        want = want + comp.decompress(p, ctx).cpu().numpy()
    assert np.array_equal(bits(got), (want / f32(2)).view(np.int32))


def _w2_worker(rank, path, outdir, dtype):
    dist.init_process_group("gloo", init_method=f"file://{path}", rank=rank, world_size=2,
                            timeout=datetime.timedelta(seconds=60))
    torch.cuda.set_device(0)
    g = spread(100003, dtype, seed=rank)[0][:100003]
    out = Allgather(AdaqCompressor(0.05), NoneMemory(), 2).step(g, "w")
    assert out.dtype == dtype and out.shape == g.shape
    np.save(os.path.join(outdir, f"r{rank}.npy"), bits(out))
    np.save(os.path.join(outdir, f"m{rank}.npy"), ops.adaq_compress(g, 0.05)[:8].cpu().numpy())
    dist.destroy_process_group()


@DTYPES
def test_world2_step(dtype):
    """Two gloo processes on one device, each under a time limit: every rank holds the rank-ordered
    average of both gradients' decodes (each with its rank's own means), rounded once."""
    with tempfile.TemporaryDirectory() as tmp:
        ctx = mp.spawn(_w2_worker, args=(os.path.join(tmp, "rdv"), tmp, dtype), nprocs=2, join=False)
        deadline = time.monotonic() + 120
        while not ctx.join(timeout=5):
            if time.monotonic() > deadline:
                for p in ctx.processes:
                    p.kill()
                pytest.fail("a rank did not finish in 120 s")
        outs = [np.load(os.path.join(tmp, f"r{r}.npy")) for r in range(2)]
        means = [np.load(os.path.join(tmp, f"m{r}.npy")).view(f32) for r in range(2)]
    ds = [ref_decode(*ref_select(spread(100003, dtype, seed=r)[1][:100003], 0.05)[:2], means[r]) for r in range(2)]
    for r in range(2):
        assert np.array_equal(outs[r], rank_sum(ds, 2, dtype)), r
