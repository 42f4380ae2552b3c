"""The microscaling codec of grace_amd/csrc/mx.hip against a numpy restatement of
include/grace_hip_mx.h in float64: each format's table of values from its (mantissa bits, bias, largest code),
the scale from the exponent of the block maximum, y = |x| 2^(127 - e) exactly, the nearest value with ties to
the even code or lo / hi and the exact fraction against the uniforms, the wire packed as a bit stream.
Everything is compared bit for bit (NaN against NaN)."""
import functools

import numpy as np
import pytest
import torch

from grace_amd import ops
from grace_amd.mx import MXCompressor, grace_from_params
from tests.device_rng import quad_uniforms

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
f32 = np.float32
FORMATS = {"fp8_e4m3": (8, 3, 7, 0x7E), "fp8_e5m2": (8, 2, 15, 0x7B), "fp6_e2m3": (6, 3, 1, 0x1F),
           "fp6_e3m2": (6, 2, 3, 0x1F), "fp4_e2m1": (4, 1, 1, 0x7)}        # bits, mantissa bits, bias, largest code
# one block, one row of a wave (256 f32, 512 bf16), a wave's chunk (1024), a workgroup's (4096), each +- 1
SIZES = [1, 31, 32, 33, 255, 257, 511, 513, 1023, 1025, 4095, 4097, 3 * 4096 + 1017]
LOOP_N = 512 * 4096 + 4096 + 33          # past kMxGridCap workgroups of 4 chunks: every wave loops, one twice


@functools.lru_cache(None)
def table(fmt):
    """(the values of the magnitude codes 0 .. largest, ascending; emax)"""
    _, M, bias, top = FORMATS[fmt]
    c = np.arange(top + 1)
    ce, cm = c >> M, c & ((1 << M) - 1)
    tab = np.where(ce > 0, (2 ** M + cm) * 2.0 ** (ce - bias - M), cm * 2.0 ** (1 - bias - M))
    return tab, int(np.floor(np.log2(tab[-1])))


def ref_encode(x, fmt, u=None):
    """(scale bytes u8[nb], codes [nb, 32]) of the f32 array x; u: the uniforms of stochastic rounding"""
    bits, _, _, top = FORMATS[fmt]
    tab, emax = table(fmt)
    nb = -(-x.size // 32)
    X = np.zeros(nb * 32, f32)
    X[:x.size] = x
    w = X.view(np.uint32).reshape(nb, 32)
    A = (w & 0x7FFFFFFF).max(axis=1)
    nanb = A >= 0x7F800000
    e = np.where(nanb, 255, np.clip((A >> 23).astype(np.int64) - emax, 0, 254))
    with np.errstate(all="ignore"):
        y = np.abs(X.astype(np.float64)).reshape(nb, 32) * 2.0 ** (127 - e)[:, None]
    y = np.minimum(np.where(nanb[:, None], 0.0, y), tab[-1])
    i = np.searchsorted(tab, y, side="right") - 1
    lo, hi = tab[i], tab[np.minimum(i + 1, top)]
    if u is None:
        up = (hi - y < y - lo) | ((hi - y == y - lo) & (i & 1 == 1))
    else:
        U = np.zeros(nb * 32)
        U[:x.size] = u
        up = U.reshape(nb, 32) * np.where(hi > lo, hi - lo, 1.0) < y - lo
    code = np.minimum(i + up, top) | ((w >> 31).astype(np.int64) << (bits - 1))
    return e.astype(np.uint8), np.where(nanb[:, None], 0, code)


def ref_wire(e, code, fmt):
    bits = FORMATS[fmt][0]
    stream = ((code.reshape(-1, 1) >> np.arange(bits)) & 1).astype(np.uint8).reshape(-1)
    parts = [e, np.packbits(stream, bitorder="little")]
    return np.concatenate([np.pad(p, (0, -p.size % 16)) for p in parts])


def ref_decode(e, code, fmt, n):
    bits = FORMATS[fmt][0]
    mag = table(fmt)[0][code & ((1 << (bits - 1)) - 1)] * 2.0 ** (e.astype(np.int64) - 127)[:, None]
    d = np.where(code >> (bits - 1) == 1, -mag, mag)
    return np.where(e[:, None] == 255, np.nan, d).astype(f32).reshape(-1)[:n]


def planted(fmt):
    """f32 blocks that reach the corners of the header: ties, saturation, subnormals, zeros, Inf, NaN, a
    denormal maximum, a clamped scale, a maximum near 2^127"""
    tab, emax = table(fmt)
    s, top, k = 2.0 ** -3, tab[-1], np.arange(32)
    mids = (tab[:-1] + tab[1:]) / 2
    sub = tab[1] * np.array([0.25, 0.49, 0.5, 0.51, 0.75, 1, 1.25, 1.5, 1.75, 2.5, 3.5, 0.0625, 1e-3, 1e-9, 2 ** -30])
    over = 2.0 ** emax * np.array([1, 1.5, 1.75, 1.875, 1.9375, 1.96875, 1.984375, 1.9921875])
    rows = [s * np.r_[mids[:31], top], s * np.r_[-mids[-31:], top], s * np.r_[over, -over, top, 1.0],
            s * np.r_[sub, -sub, top], np.r_[np.zeros(7), -0.0], np.r_[0.0, -0.0, 1.0, -1.0], np.r_[1.0, np.inf, 2.0],
            np.r_[-3.0, np.nan, 5.0, -np.inf], k * 2.0 ** -133, np.r_[np.arange(1, 20) * 2.0 ** -149, -7 * 2.0 ** -140],
            (1 + k / 32) * 2.0 ** (emax - 128) * np.where(k % 3 == 0, -2.0 ** -(k % 7), 1.0),   # E = emax - 1: e = 0
            np.r_[1.5 * 2.0 ** 127, -mids[:31] * 2.0 ** 120]]
    out = np.zeros((len(rows), 32))
    for r, row in zip(out, rows):
        r[:row.size] = row
    return out.astype(f32).reshape(-1)


@functools.lru_cache(None)
def gradient(n, dtype, fmt):
    """randn scaled per 100-element stretch by 1e-6 .. 1e3 behind the planted blocks: (device tensor, its
    values as f32 numpy)"""
    g = torch.Generator().manual_seed(n)
    x = torch.randn(n, generator=g) * 10.0 ** ((torch.arange(n) // 100 % 10) - 6).float()
    p = torch.from_numpy(planted(fmt))[:n]
    x[:p.numel()] = p
    x = x.to(dtype)
    return x.to(DEV), x.float().numpy()


def same(got, want):
    g, w = got.detach().cpu().float().numpy().reshape(-1), np.asarray(want, f32).reshape(-1)
    nan = np.isnan(w)
    return np.array_equal(np.isnan(g), nan) and np.array_equal(g.view(np.int32)[~nan], w.view(np.int32)[~nan])


def uniforms(seed, n):
    i = np.arange(n, dtype=np.int64)
    return quad_uniforms(seed, i // 4 * 4, i % 4)


def check(xd, x, fmt, rounding, seed=11):
    u = uniforms(seed, x.size) if rounding == "stochastic" else None
    e, code = ref_encode(x, fmt, u)
    got = ops.mx_compress(xd, fmt, rounding, seed=seed).cpu().numpy()
    want = ref_wire(e, code, fmt)
    assert got.size == want.size == ops.mx_payload_bytes(x.size, fmt)
    assert np.array_equal(got, want)
    out = ops.mx_step_w1(xd, fmt, rounding, seed=seed)
    assert out.dtype == xd.dtype and out.shape == xd.shape
    assert same(out, ref_decode(e, code, fmt, x.size))      # exact in bf16 too: at most 4 significant bits
    return u, want


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("rounding", ops.MX_ROUNDINGS)
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_compress_and_step(dtype, fmt, rounding, n):
    xd, x = gradient(n, dtype, fmt)
    u, want = check(xd, x, fmt, rounding)
    if u is not None:       # the injected uniforms give the seeded call's bytes
        got = ops.mx_compress(xd, fmt, rounding, u=torch.from_numpy(u).to(DEV))
        assert np.array_equal(got.cpu().numpy(), want)


@pytest.mark.parametrize("fmt,rounding,dtype", [(f, ops.MX_ROUNDINGS[i & 1], (F32, BF16)[i >> 1 & 1])
                                                for i, f in enumerate(FORMATS)])
def test_a_wave_loops_over_its_chunks(fmt, rounding, dtype):
    xd, x = gradient(LOOP_N, dtype, fmt)
    check(xd, x, fmt, rounding)


@pytest.mark.parametrize("fmt", ["fp8_e5m2", "fp6_e2m3", "fp4_e2m1"])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_pointers_off_the_16_byte_grid(dtype, fmt):
    xd, x = gradient(4097, dtype, fmt)
    u = uniforms(11, 4097)
    assert xd.data_ptr() % 16 == 0
    check(xd[1:], x[1:], fmt, "nearest")
    got = ops.mx_compress(xd[1:], fmt, "stochastic", u=torch.from_numpy(u).to(DEV)[1:])
    assert np.array_equal(got.cpu().numpy(), ref_wire(*ref_encode(x[1:], fmt, u[1:]), fmt))


@pytest.mark.parametrize("out_dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("n", [33, 1025, 4097])          # nb = 2, 33, 129: scale padding and ragged groups
@pytest.mark.parametrize("world", [1, 2, 3])
@pytest.mark.parametrize("fmt", FORMATS)
def test_decode_aggregate(fmt, world, n, out_dtype):
    big = gradient(3 * 4096 + 1017, F32, fmt)
    xs = [(xd[lo:lo + n], x[lo:lo + n])           # rank 0 holds the planted blocks; rank 1 is off the 16-B grid
          for lo, (xd, x) in ((0, gradient(4097, F32, fmt)), (4099, big), (8192, big))][:world]
    pay = torch.cat([ops.mx_compress(xd, fmt) for xd, _ in xs])
    acc = None
    with np.errstate(all="ignore"):
        for _, x in xs:
            d = ref_decode(*ref_encode(x, fmt), fmt, n)
            acc = d if acc is None else acc + d
        acc = acc / f32(3.0)
    got = ops.mx_decode_aggregate(pay, world, n, fmt, divisor=3.0, out_dtype=out_dtype)
    assert got.dtype == out_dtype and same(got, torch.from_numpy(acc).to(out_dtype).float().numpy())


def test_stochastic_rounding_is_unbiased():
    """4.5 between FP4's 4 and 6 (X = 1): up with p = 1/4; the share of 2^16 draws is binomial, so within
    5 sigma = 5 sqrt(p (1 - p) / N) of p"""
    N, p = 1 << 16, 0.25
    pay = ops.mx_compress(torch.full((N,), 4.5, device=DEV), "fp4_e2m1", "stochastic", seed=2024).cpu().numpy()
    codes = pay[N // 32:]
    nib = np.stack([codes & 15, codes >> 4], axis=1).reshape(-1)[:N]
    assert set(np.unique(nib)) == {6, 7} and (pay[:N // 32] == 127).all()
    assert abs((nib == 7).mean() - p) < 5 * np.sqrt(p * (1 - p) / N)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("rounding", ops.MX_ROUNDINGS)
def test_grace_from_params_steps_through_the_fused_step(rounding, dtype):
    comm = grace_from_params({'compressor': 'mx', 'memory': 'none', 'communicator': 'allgather', 'world_size': 1,
                              'format': 'fp6_e3m2', 'rounding': rounding})
    assert isinstance(comm.compressor, MXCompressor) and comm.compressor.format == 'fp6_e3m2'
    xd = gradient(4097, dtype, 'fp6_e3m2')[0][:4096].view(64, 64)
    out = comm.step(xd, "w")
    seed = ops.step_seed("mx", 0, "w", 1)
    assert out.dtype == dtype and out.shape == xd.shape
    assert same(out, ops.mx_step_w1(xd, 'fp6_e3m2', rounding, seed=seed).float().cpu().numpy())
