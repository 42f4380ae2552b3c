"""The quantile-bucket quantiser of grace_amd/csrc/sketch.hip against a numpy reference of
include/grace_hip_sketch.h, stage by stage: the edges bit for bit (np.sort and the integer rank
formula), the codes bit for bit given the device's edges (np.searchsorted), the means within
2^-52 * sum|x_i| + 2^-23 * |mean| of math.fsum's (an f64 sum in any order, then one rounding to f32), and
the decode and the step exactly means[code] of the means the device returned."""
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

from grace_amd import ops
from grace_amd.dist.communicator.allgather import Allgather
from grace_amd.dist.memory.none import NoneMemory
from grace_amd.sketch import SketchCompressor, grace_from_params

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
f32 = np.float32
DTYPES = pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
QS = pytest.mark.parametrize("q", [2, 16, 17, 255, 256])
# sketch.hip: a select workgroup takes 1024 * 4 f32 (8 bf16) elements a sweep, so N_GROUPS is past one
# workgroup's share; its grid stops at 512 workgroups and the encode's and decode's at 2048 of 256 threads,
# so one sweep of any of them is 2^21 f32 or 2^22 bf16 elements and N_SWEEPS is past all of them
N_GROUPS, N_SWEEPS = 3 * 8192 + 5, (1 << 22) + 4099


@functools.lru_cache(None)
def data(kind, n, dtype):
    """(device tensor of n + 1 elements, its values as f32 numpy): the tests take [:n] or [1:]"""
    rng = np.random.default_rng(n + len(kind))
    m = n + 1
    if kind == "normal":            # most ranks fall in a few top-digit bins
        x = rng.standard_normal(m) * 1e-3
    elif kind == "five":            # ties, empty buckets and both zeros
        x = np.array([-1.5, 0.0, -0.0, 2.0, 3e-5])[rng.integers(0, 5, m)]
    elif kind == "ramp":            # f32: every rank shares its prefix until the last digits; bf16: all equal
        x = 1.0 + (np.arange(m) % 4096) * 2.0 ** -23
    elif kind == "wide":            # prefixes live in every exponent
        x = rng.standard_normal(m) * 2.0 ** rng.uniform(-40, 20, m)
    else:                           # "inf"
        x = rng.standard_normal(m)
        x[rng.integers(0, m, 6)] = [np.inf, -np.inf, np.inf, np.inf, -np.inf, 0.0]
    t = torch.from_numpy(x.astype(f32)).to(dtype)
    return t.to(DEV), t.float().numpy()


def bits(t):
    t = t.detach().cpu().contiguous().reshape(-1)
    return t.view(torch.int16 if t.dtype == BF16 else torch.int32).numpy()


def unpack(codes, n, q):
    c = codes.cpu().numpy()
    if q <= 16:
        c = np.stack([c & 15, c >> 4], axis=1).reshape(-1)
        assert not c[n:].any()      # the unused high nibble of an odd n
    return c[:n].astype(np.int64)


def check_means(got, x, order, counts, q):
    """every mean against math.fsum over its bucket (order: the elements sorted by code, stably)"""
    start = 0
    for b in range(q):
        v = x[order[start:start + counts[b]]].astype(np.float64)
        start += counts[b]
        want = math.fsum(v) / len(v) if len(v) else 0.0
        with np.errstate(invalid="ignore"):
            err, bound = abs(float(got[b]) - want), 2.0 ** -52 * float(np.abs(v).sum()) + 2.0 ** -23 * abs(want)
        assert got[b] == f32(want) or err <= bound, (b, got[b], want, bound)


def check(xd, x, q, codes_out=None):
    n = x.size
    x = x + f32(0)                  # a zero of either sign is +0.0
    want_e = np.sort(x)[[j * (n - 1) // q for j in range(q + 1)]]
    edges = ops.sketch_edges(xd, q)
    assert np.array_equal(bits(edges), want_e.view(np.int32))
    codes, means = ops.sketch_compress(xd, q, out=codes_out)
    want_c = np.searchsorted(edges.cpu().numpy()[1:q], x, side="right")
    assert codes.numel() == ops.sketch_code_bytes(n, q) and np.array_equal(unpack(codes, n, q), want_c)
    m_step, out = ops.sketch_step_w1(xd, q)
    order, counts = np.argsort(want_c, kind="stable"), np.bincount(want_c, minlength=q)
    for m in (means, m_step):
        check_means(m.cpu().numpy(), x, order, counts, q)
    assert out.dtype == xd.dtype and out.shape == xd.shape
    assert np.array_equal(bits(out), bits(torch.from_numpy(f32(0) + m_step.cpu().numpy()[want_c]).to(xd.dtype)))
    dec = ops.sketch_decode_aggregate(codes, means, 1, n, q, out_dtype=xd.dtype)
    assert np.array_equal(bits(dec), bits(torch.from_numpy(f32(0) + means.cpu().numpy()[want_c]).to(xd.dtype)))


@QS
@DTYPES
@pytest.mark.parametrize("n", [1, 5, 257, 4099, N_GROUPS, N_SWEEPS])
def test_normal_gradient_at_every_size(n, dtype, q):
    xd, x = data("normal", n, dtype)
    check(xd[:n], x[:n], q)


@QS
@DTYPES
@pytest.mark.parametrize("kind", ["five", "ramp", "wide", "inf"])
def test_hard_distributions(kind, dtype, q):
    xd, x = data(kind, N_GROUPS, dtype)
    check(xd[:N_GROUPS], x[:N_GROUPS], q)


@pytest.mark.parametrize("q", [16, 256])
@DTYPES
def test_pointers_off_the_vector_grid(dtype, q):
    """the gradient one element, and the codes one byte, past a 16-byte boundary"""
    xd, x = data("wide", N_GROUPS, dtype)
    assert xd.data_ptr() % 16 == 0
    check(xd[1:], x[1:], q)
    buf = torch.zeros(ops.sketch_code_bytes(N_GROUPS, q) + 2, dtype=torch.uint8, device=DEV)
    check(xd[:N_GROUPS], x[:N_GROUPS], q, codes_out=buf[1:-1])
    assert int(buf[0]) == 0 and int(buf[-1]) == 0


@pytest.mark.parametrize("out_dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("divisor", [1, 3])
@pytest.mark.parametrize("pad", [8, 3], ids=["rows_aligned", "rows_odd"])
@pytest.mark.parametrize("world,q,n", [(3, 16, 4099), (3, 200, 4099), (65, 256, 257)])   # 65 * 256: means not in LDS
def test_decode_aggregate(world, q, n, pad, divisor, out_dtype):
    rng = np.random.default_rng(n + world + q)
    row = ops.sketch_code_bytes(n, q)
    stride = -(-row // 8) * 8 + 8 if pad == 8 else row + pad     # every row 8-byte aligned, or not
    c = rng.integers(0, q, (world, n))
    means = rng.standard_normal((world, q)).astype(f32)
    wire = np.zeros((world, stride), np.uint8)
    if q <= 16:
        cp = np.concatenate([c, np.zeros((world, 2 * row - n), np.int64)], axis=1)
        wire[:, :row] = cp[:, 0::2] | (cp[:, 1::2] << 4)
    else:
        wire[:, :row] = c
    acc = np.zeros(n, f32)
    for w in range(world):
        acc = acc + means[w][c[w]]
    if divisor != 1:
        acc = acc / f32(divisor)
    got = ops.sketch_decode_aggregate(torch.from_numpy(wire.reshape(-1)[:(world - 1) * stride + row].copy()).to(DEV),
                                      torch.from_numpy(means).reshape(-1).to(DEV), world, n, q, divisor=divisor,
                                      out_dtype=out_dtype, code_stride=stride)
    assert got.dtype == out_dtype and np.array_equal(bits(got), bits(torch.from_numpy(acc).to(out_dtype)))


@DTYPES
def test_allgather_step_world1_and_from_params(dtype):
    xd = data("normal", 4099, dtype)[0][:4096].view(64, 64)
    for comm in (Allgather(SketchCompressor(17), NoneMemory(), 1),
                 grace_from_params({'compressor': 'sketch', 'memory': 'none', 'communicator': 'allgather',
                                    'world_size': 1, 'quantiles': 17})):
        out = comm.step(xd, "w")
        assert out.dtype == dtype and out.shape == xd.shape
        assert np.array_equal(bits(out), bits(ops.sketch_step_w1(xd, 17)[1]))


def test_decode_aggregate_gathered_equals_the_decompress_loop():
    comp = SketchCompressor(16)
    pay = [comp.compress(data("normal", n, F32)[0][:4099], "w") for n in (4099, N_GROUPS)]
    ctx = pay[0][1]
    got = comp.decode_aggregate_gathered([torch.cat([p[0][j] for p in pay]) for j in range(2)], ctx, 2)
    want = np.zeros(4099, f32)
    for p, _ in pay:
        want = want + comp.decompress(p, ctx).cpu().numpy()
    assert np.array_equal(bits(got), (want / f32(2)).view(np.int32))


def _w2_worker(rank, path, outdir, dtype):
    dist.init_process_group("gloo", init_method=f"file://{path}", rank=rank, world_size=2,
                            timeout=datetime.timedelta(seconds=60))
    torch.cuda.set_device(0)
    gs = [data("normal", 100003 + r, dtype)[0][:100003] for r in range(2)]
    out = Allgather(SketchCompressor(16), NoneMemory(), 2).step(gs[rank], "w")
    assert out.dtype == dtype and out.shape == gs[rank].shape
    acc = np.zeros(100003, f32)
    for g in gs:                    # both ranks' payloads, decoded and summed on the host in rank order
        codes, means = ops.sketch_compress(g, 16)
        acc = acc + means.cpu().numpy()[unpack(codes, 100003, 16)]
    np.savez(os.path.join(outdir, f"r{rank}.npz"), out=bits(out), ref=bits(torch.from_numpy(acc / f32(2)).to(dtype)))
    dist.destroy_process_group()


@DTYPES
def test_world2_step(dtype):
    """Two gloo processes on one device, each under a time limit: every rank holds the rank-ordered
    average of both payloads' decodes, rounded once."""
    with tempfile.TemporaryDirectory() as tmp:
        ctx = mp.spawn(_w2_worker, args=(os.path.join(tmp, "rdv"), tmp, dtype), nprocs=2, join=False)
        deadline = time.monotonic() + 120
        while not ctx.join(timeout=5):
            if time.monotonic() > deadline:
                for p in ctx.processes:
                    p.kill()
                pytest.fail("a rank did not finish in 120 s")
        zs = [dict(np.load(os.path.join(tmp, f"r{r}.npz"))) for r in range(2)]
    for r in range(2):
        assert np.array_equal(zs[r]["out"], zs[r]["ref"]), r
    assert np.array_equal(zs[0]["out"], zs[1]["out"])
