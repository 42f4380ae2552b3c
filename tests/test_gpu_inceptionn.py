"""The error-bounded variable-width codec of grace_amd/csrc/inceptionn.hip against a numpy
restatement of include/grace_hip_inceptionn.h, bit for bit: every tile's bytes wherever the encoder put
it, the partition of the payload, and the decode, the world-1 step and the rank-ordered f32 sum.  The
codec is integer work and the floors are taken in f64, where they are exact, so no tolerance occurs."""
import datetime
import functools
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
from grace_amd.inceptionn import InceptionnCompressor, grace_from_params

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
f32, T = np.float32, 4096
DTYPES = pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
BS = pytest.mark.parametrize("b", [1, 10, 14])
# inceptionn.hip: encode and decode launch one workgroup a tile, uncapped; only the world-1 step's grid stops,
# at 2048 workgroups of 256 threads and 16 B a thread, so one sweep of it is 2^21 f32 or 2^22 bf16 elements
# and N_SWEEP is past it
N_ODD, N_SWEEP = 3 * T + 5, (1 << 22) + 4099


def bits(t):
    t = t.detach().cpu().contiguous().reshape(-1)
    return t.view(torch.int16 if t.dtype == BF16 else torch.int32).numpy()


def on_device(x, dtype):
    """(device tensor of x in dtype, its values widened to f32 numpy)"""
    t = torch.from_numpy(np.asarray(x, f32)).to(dtype)
    return t.to(DEV), t.float().numpy()


@functools.lru_cache(None)
def spread(n, dtype, seed=0):
    """n + 1 elements with magnitudes over 2^-30 .. 2^3, so that all four tags occur in most tiles"""
    rng = np.random.default_rng(n + seed)
    return on_device(rng.choice([-1.0, 1.0], n + 1) * (1 + rng.random(n + 1)) * 2.0 ** rng.integers(-30, 3, n + 1), dtype)


def ref_codes(x, b):
    """the header's table: (tag, code, decoded value) of every element of the f32 array x"""
    E = 127 - b
    mid = E + (b + 1) // 2
    u = x.view(np.uint32)
    e, s, a = (u >> 23) & 255, (u >> 31).astype(np.int64), np.abs(x.astype(np.float64))
    tag = (e >= E).astype(np.int64) + (e >= mid) + (e >= 127)
    with np.errstate(invalid="ignore"):
        q = np.where(tag == 2, np.floor(a * 2.0 ** 15), np.where(tag == 1, np.floor(a * 2.0 ** (134 - mid)), 0)).astype(np.int64)
        d = (1 - 2 * s) * q * np.where(tag == 2, 2.0 ** -15, 2.0 ** (mid - 134))
    code = np.where(tag == 2, s << 15 | q, s << 7 | q)
    return tag, code, np.where(tag == 3, x, d.astype(f32))


def ref_tiles(x, b):
    """the bytes of every tile of x, as the header states them"""
    tag, code, _ = ref_codes(x, b)
    tiles = []
    for i in range(0, x.size, T):
        t, c, v = tag[i:i + T], code[i:i + T], x[i:i + T]
        t4 = np.concatenate([t, np.zeros(-t.size % 64, np.int64)]).reshape(-1, 4)
        raw = b"".join([(t4[:, 0] | t4[:, 1] << 2 | t4[:, 2] << 4 | t4[:, 3] << 6).astype(np.uint8).tobytes(),
                        v[t == 3].tobytes(), c[t == 2].astype(np.uint16).tobytes(), c[t == 1].astype(np.uint8).tobytes()])
        tiles.append(raw + bytes(-len(raw) % 16))
    return tiles


def ref_payload(x, b):
    """a payload with its tiles placed in reverse order"""
    tiles = ref_tiles(x, b)
    words = np.zeros(-(-(len(tiles) + 1) // 4) * 4, np.uint32)
    body = b""
    for i in reversed(range(len(tiles))):
        words[1 + i] = (words.nbytes + len(body)) // 16
        body += tiles[i]
    words[0] = (words.nbytes + len(body)) // 16
    return words.tobytes() + body


def check(xd, x, b):
    n = x.size
    cap = ops.inceptionn_capacity_bytes(n)
    ntiles = -(-n // T)
    assert cap == 16 * (-(-(ntiles + 1) // 4)) + sum(16 * (-(-m // 64) + -(-m // 4)) for m in [T] * (n // T) + [n % T])
    payload = ops.inceptionn_compress(xd, b)
    total = ops.inceptionn_payload_bytes(payload)
    assert payload.numel() == cap and total <= cap
    raw = payload[:total].cpu().numpy().tobytes()
    words = np.frombuffer(raw, np.uint32, -(-(ntiles + 1) // 4) * 4)
    assert words[0] * 16 == total and not words[1 + ntiles:].any()
    tiles = ref_tiles(x, b)
    spans = [(0, words.nbytes)]
    for i, want in enumerate(tiles):
        off = int(words[1 + i]) * 16
        assert raw[off:off + len(want)] == want, i
        spans.append((off, off + len(want)))
    spans.sort()
    assert spans[-1][1] == total and all(p[1] == q[0] for p, q in zip(spans, spans[1:]))   # a partition of [0, total)
    want = bits(torch.from_numpy(ref_codes(x, b)[2]).to(xd.dtype))
    dec = ops.inceptionn_decode_aggregate(payload[:total], 1, n, b, out_dtype=xd.dtype)
    step = ops.inceptionn_step_w1(xd, b)
    assert dec.dtype == step.dtype == xd.dtype and step.shape == xd.shape
    assert np.array_equal(bits(dec), want) and np.array_equal(bits(step), want)
    return total


@BS
@DTYPES
@pytest.mark.parametrize("n", [1, 63, 64, 65, 4095, 4096, 4097, N_ODD, N_SWEEP])
def test_encode_at_every_size(n, dtype, b):
    xd, x = spread(n, dtype)
    check(xd[:n], x[:n], b)


@BS
@DTYPES
def test_edge_values(dtype, b):
    n, mid = 4099, 127 - b + (b + 1) // 2
    xd, x = on_device(np.full(n, 2.0 ** (126 - 127 - b)), dtype)              # every element tag 0
    assert check(xd, x, b) == 16 + 16 * 64 + 16
    xd, x = on_device(np.resize([1.0, -3.5, 1e30, -np.inf], n), dtype)       # every element tag 3
    assert check(xd, x, b) == ops.inceptionn_capacity_bytes(n)
    edges = np.array([1.0, 2.0 ** -b, 2.0 ** (mid - 127)])
    below = np.nextafter(edges.astype(f32), f32(0)) if dtype == F32 else edges * (1 - 2.0 ** -8)
    special = np.concatenate([[0.0, -0.0, 1e-40, -1e-40, np.inf, -np.inf], [np.nan] * (dtype == F32),
                              edges, -edges, below, -below]).astype(f32)
    xd, x = on_device(np.resize(special, n), dtype)
    check(xd, x, b)


@DTYPES
def test_gradient_off_the_vector_grid(dtype):
    """the gradient one element past a 16-byte boundary"""
    xd, x = spread(N_ODD, dtype)
    assert xd.data_ptr() % 16 == 0
    check(xd[1:], x[1:], 10)


@pytest.mark.parametrize("out_dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("divisor", [1, 3])
@pytest.mark.parametrize("world", [3, 65])
def test_decode_across_ranks(world, divisor, out_dtype):
    """numpy-written payloads of different lengths, padded to the longest, the tiles in reverse order: the
    decoder follows the directory"""
    n, b = 2 * T + 5, 10
    xs = [spread(n, F32, seed=w)[1][:n] * f32(2.0 ** -(w % 7)) for w in range(world)]
    pays = [ref_payload(x, b) for x in xs]
    stride = max(len(p) for p in pays)
    assert len(set(len(p) for p in pays)) > 1
    wire = np.frombuffer(b"".join(p + bytes(stride - len(p)) for p in pays), np.uint8)
    acc = np.zeros(n, f32)
    for x in xs:
        acc = acc + ref_codes(x, b)[2]
    if divisor != 1:
        acc = acc / f32(divisor)
    got = ops.inceptionn_decode_aggregate(torch.from_numpy(wire.copy()).to(DEV), world, n, b, divisor=divisor,
                                          out_dtype=out_dtype)
    assert got.dtype == out_dtype and np.array_equal(bits(got), bits(torch.from_numpy(acc).to(out_dtype)))


def test_a_tile_outside_its_rank_is_skipped():
    """the tile placed last leaves a stride cut by 16 bytes, and one whose entry points into the header is
    refused: both contribute zeros, the other tiles decode"""
    n, b = 2 * T + 5, 10
    x = spread(n, F32)[1][:n]
    want = ref_codes(x, b)[2]
    pay = np.frombuffer(ref_payload(x, b), np.uint8).copy()
    got = ops.inceptionn_decode_aggregate(torch.from_numpy(pay).to(DEV), 1, n, b, stride=pay.size - 16)
    assert np.array_equal(bits(got), np.concatenate([np.zeros(T, f32), want[T:]]).view(np.int32))
    pay.view(np.uint32)[2] = 0
    got = ops.inceptionn_decode_aggregate(torch.from_numpy(pay).to(DEV), 1, n, b)
    assert np.array_equal(bits(got), np.concatenate([want[:T], np.zeros(T, f32), want[2 * T:]]).view(np.int32))


@DTYPES
def test_allgather_step_world1_and_from_params(dtype):
    xd, x = spread(4099, dtype)
    xd, want = xd[:4096].view(64, 64), bits(torch.from_numpy(ref_codes(x[:4096], 12)[2]).to(dtype))
    for comm in (Allgather(InceptionnCompressor(12), NoneMemory(), 1),
                 grace_from_params({'compressor': 'inceptionn', 'memory': 'none', 'communicator': 'allgather',
                                    'world_size': 1, 'bound_bits': 12})):
        out = comm.step(xd, "w")
        assert out.dtype == dtype and out.shape == xd.shape and np.array_equal(bits(out), want)


def test_decode_aggregate_variable_equals_the_decompress_loop():
    comp = InceptionnCompressor(10)
    pay = [comp.compress(spread(4099, F32, seed=s)[0][:4099] * 2.0 ** -s, "w") for s in (0, 5)]
    ctx, sizes = pay[0][1], [[p[0][0].numel()] for p in pay]
    assert sizes[0] != sizes[1]
    rows = torch.zeros(2, max(s[0] for s in sizes), dtype=torch.uint8, device=DEV)
    for r, (p, _) in enumerate(pay):
        rows[r, :sizes[r][0]] = p[0]
    got = comp.decode_aggregate_variable([rows.view(-1)], sizes, ctx, 2)
    want = np.zeros(4099, f32)
    for p, _ in pay:
        want = want + comp.decompress(p, ctx).cpu().numpy()
    assert np.array_equal(bits(got), (want / f32(2)).view(np.int32))


def _w2_worker(rank, path, outdir, dtype):
    dist.init_process_group("gloo", init_method=f"file://{path}", rank=rank, world_size=2,
                            timeout=datetime.timedelta(seconds=60))
    torch.cuda.set_device(0)
    g = spread(100003, dtype, seed=rank)[0][:100003]
    out = Allgather(InceptionnCompressor(10), NoneMemory(), 2).step(g, "w")
    assert out.dtype == dtype and out.shape == g.shape
    np.save(os.path.join(outdir, f"r{rank}.npy"), bits(out))
    dist.destroy_process_group()


@DTYPES
def test_world2_step(dtype):
    """Two gloo processes on one device, each under a time limit: every rank holds the rank-ordered
    average of both gradients' decodes, rounded once."""
    with tempfile.TemporaryDirectory() as tmp:
        ctx = mp.spawn(_w2_worker, args=(os.path.join(tmp, "rdv"), tmp, dtype), nprocs=2, join=False)
        deadline = time.monotonic() + 120
        while not ctx.join(timeout=5):
            if time.monotonic() > deadline:
                for p in ctx.processes:
                    p.kill()
                pytest.fail("a rank did not finish in 120 s")
        outs = [np.load(os.path.join(tmp, f"r{r}.npy")) for r in range(2)]
    acc = np.zeros(100003, f32)
    for r in range(2):
        acc = acc + ref_codes(spread(100003, dtype, seed=r)[1][:100003], 10)[2]
    for r in range(2):
        assert np.array_equal(outs[r], bits(torch.from_numpy(acc / f32(2)).to(dtype))), r
