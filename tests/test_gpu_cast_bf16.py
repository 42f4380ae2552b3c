"""The natural, cnat and fp16 kernels of grace_amd/csrc/cast.hip on bfloat16.

Sizes: ragged ones around the 8-element group, 4099, 65,537, 262,149, 1,048,579 and WRAP = 2^23 + 5,
just past one trip of the capped grid (4096 workgroups x 256 lanes x 8 elements).  Views: every
operand aligned, or every operand starting 1, 2 or 4 elements into its buffer (2-, 4- and 8-byte
aligned bf16: the guarded path); past 65,537 the aligned and the 1-element views only.  Every operand
sits between sentinels that must survive, and inputs must come back unchanged.

Inputs are bf16-representable: normals with ±0, bf16 denormals, ±inf and NaN planted, plus the f16
range edges and the exponents at both clip ends of the natural codecs.  Codes are compared with the
oracle on the widened input under injected randoms, and with the f32 entry point on ``g.float()``
under the same seed for the device generator: equal bits.  Steps and decodes are compared with the
f32 kernel's result through torch's CPU cast: equal 16-bit patterns, NaN-ness only at a NaN."""
import functools

import numpy as np
import pytest
import torch

from grace_amd import _lib, ops
from oracle import grace_oracle as O
from tests import cast_bf16_util as U

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, F16, F32, U8, I32 = torch.bfloat16, torch.float16, torch.float32, torch.uint8, torch.int32
WRAP = (1 << 23) + 5
SIZES = (1, 3, 5, 7, 8, 9, 15, 17, 4099, 65537, 262149, 1048579, WRAP)
GUARD = 16      # sentinel elements either side: 16 B or more of every element type, so `off` alone misaligns
SENT = {BF16: 0x4D4D, F16: 0x4D4D, U8: 0xA5, I32: 0x5A5A5A5A, F32: 0x4D4D4D4D}      # bit patterns
NPINT = {BF16: np.uint16, F16: np.uint16, U8: np.uint8, I32: np.uint32, F32: np.uint32}
SIGNED = {BF16: torch.int16, F16: torch.int16, U8: torch.uint8, I32: torch.int32, F32: torch.int32}


def cases(sizes=SIZES):
    return [pytest.param(n, off, id=f"n{n}-off{off}") for n in sizes for off in ((0, 1, 2, 4) if n <= 65537 else (0, 1))]


class Slot:
    """n elements of `dtype` starting `off` elements into an aligned buffer, sentinels either side.
    Contents go in and come out as unsigned bit patterns (numpy)."""

    def __init__(self, n, dtype, off, bits=None):
        self.dtype, self.n, self.lo = dtype, n, GUARD + off
        raw = np.full(n + 2 * GUARD + 8, SENT[dtype], dtype=NPINT[dtype])
        if bits is not None:
            raw[self.lo:self.lo + n] = bits
        self.buf = torch.from_numpy(raw.view(raw.dtype.str.replace("u", "i")) if dtype != U8 else raw).to(DEV)
        self.buf = self.buf.view(dtype)
        self.t = self.buf[self.lo:self.lo + n]
        assert self.buf.data_ptr() % 16 == 0 and self.t.data_ptr() % 16 == (self.lo * self.t.element_size()) % 16

    def all_bits(self):
        return self.buf.view(SIGNED[self.dtype]).cpu().numpy().view(NPINT[self.dtype])

    def bits(self):
        return self.all_bits()[self.lo:self.lo + self.n]

    def guards_intact(self):
        b = self.all_bits()
        return bool((b[:self.lo] == SENT[self.dtype]).all() and (b[self.lo + self.n:] == SENT[self.dtype]).all())


@functools.lru_cache(maxsize=None)
def grad_bits(n, seed=0):
    """bf16 patterns [n], read-only: normals scaled over a few exponents with the specials, the f16
    edges and the natural clip ends planted at both ends and inside (n < 24: a run of the pool)."""
    pool = U.narrow(np.concatenate([U.SPECIALS, U.FP16_EDGES, -U.FP16_EDGES[:2], U.NATURAL_EDGES]))
    if n < 24:
        b = pool[(np.arange(n) + 5 * seed + n) % pool.size].copy()
    else:
        rng = np.random.default_rng(100 + seed + n % 1000)
        b = U.narrow(rng.standard_normal(n).astype(np.float32) * np.exp2(rng.integers(-20, 4, n)).astype(np.float32))
        for base in (0, n // 3, n // 2 + 1, n - pool.size):
            b[base:base + pool.size] = pool
    b.setflags(write=False)
    return b


@functools.lru_cache(maxsize=None)
def randoms(n):
    rng = np.random.default_rng(n % 977)
    ri = rng.integers(0, 0x7FFFFF, n).astype(np.int32)
    ri[::5] = 0x7FFFFE
    ri[1::7] = 0
    u = rng.random(n).astype(np.float32)
    u[::9] = 0.0
    return ri, u


def f32_dev(bits):
    return torch.from_numpy(U.widen(bits)).to(DEV)


def torch_round(t):
    """An f32 device result through torch's CPU cast, as bf16 patterns."""
    return t.cpu().to(BF16).view(torch.int16).numpy().view(np.uint16)


# ----------------------------------------------------------------------------- encoders
@pytest.mark.parametrize("n,off", cases())
def test_natural_codes(n, off):
    bits = grad_bits(n)
    ri, _ = randoms(n)
    x, r, c = Slot(n, BF16, off, bits), Slot(n, I32, off, ri.view(np.uint32)), Slot(n, U8, off)
    ops.natural_compress(x.t, rand_int=r.t, out=c.t)
    want = O.natural_compress(U.widen(bits), ri)
    assert np.array_equal(c.bits(), want)
    assert c.guards_intact() and x.guards_intact() and np.array_equal(x.bits(), bits)
    # the device generator: the f32 entry point's codes for g.float() under the same seed and xoff
    for seed, xoff in ((12345, 0), (-7, 4096)):
        c2 = Slot(n, U8, off)
        ops.natural_compress(x.t, seed=seed, xoff=xoff, out=c2.t)
        ref = ops.natural_compress(f32_dev(bits), seed=seed, xoff=xoff)
        assert np.array_equal(c2.bits(), ref.cpu().numpy()) and c2.guards_intact()


@pytest.mark.parametrize("n,off", cases())
def test_cnat_codes(n, off):
    bits = grad_bits(n, 1)
    _, u = randoms(n)
    x, r, c = Slot(n, BF16, off, bits), Slot(n, F32, off, u.view(np.uint32)), Slot(n, U8, off)
    ops.cnat_compress(x.t, rand=r.t, out=c.t)
    assert np.array_equal(c.bits(), O.cnat_compress(U.widen(bits), u))
    assert c.guards_intact() and x.guards_intact() and np.array_equal(x.bits(), bits)
    cd = Slot(n, U8, off)
    ops.cnat_compress(x.t, deterministic=True, out=cd.t)
    assert np.array_equal(cd.bits(), O.cnat_compress(U.widen(bits))) and cd.guards_intact()
    for seed, xoff in ((12345, 0), (-7, 4096)):
        c2 = Slot(n, U8, off)
        ops.cnat_compress(x.t, seed=seed, xoff=xoff, out=c2.t)
        ref = ops.cnat_compress(f32_dev(bits), seed=seed, xoff=xoff)
        assert np.array_equal(c2.bits(), ref.cpu().numpy()) and c2.guards_intact()


@pytest.mark.parametrize("n,off", cases())
def test_fp16_payload(n, off):
    bits = grad_bits(n, 2)
    x, h = Slot(n, BF16, off, bits), Slot(n, F16, off)
    ops.fp16_compress(x.t, out=h.t)
    with np.errstate(all="ignore"):
        want = O.fp16_compress(U.widen(bits)).view(np.uint16)
    got = h.bits()
    nan = np.isnan(want.view(np.float16))
    assert np.array_equal(np.isnan(got.view(np.float16)), nan) and np.array_equal(got[~nan], want[~nan])
    ref = ops.fp16_compress(f32_dev(bits)).view(torch.int16).cpu().numpy().view(np.uint16)
    assert np.array_equal(got, ref)                                   # the f32 entry point's bits, NaNs included
    assert h.guards_intact() and x.guards_intact() and np.array_equal(x.bits(), bits)


# ----------------------------------------------------------------------------- the world-1 step
@pytest.mark.parametrize("n,off", cases())
def test_cast_step_w1(n, off):
    bits = grad_bits(n, 3)
    x = Slot(n, BF16, off, bits)
    xf = f32_dev(bits)
    for mode, seed in ((0, 2024), (1, -3), (2, 0), (3, 0)):
        o = Slot(n, BF16, off)
        _lib.call("grace_cast_step_w1_bf16", x.t.data_ptr(), n, mode, ops.seed64(seed), o.t.data_ptr(), ops._stream())
        want = torch_round(ops.cast_step_w1(xf, mode, seed))
        assert U.same_bf16(o.bits(), want) is None, (mode, U.same_bf16(o.bits(), want))
        assert o.guards_intact(), mode
        if mode >= 2:   # no generator: the numpy restatement as well
            assert U.same_bf16(o.bits(), U.cast_step(bits, mode)) is None, mode
    assert x.guards_intact() and np.array_equal(x.bits(), bits)
    if off == 0:
        out = ops.cast_step_w1(x.t.view(1, n), 3, 0)
        assert out.dtype == BF16 and out.shape == (1, n) and U.same_bf16(torch_round(out.float()), want) is None


# ----------------------------------------------------------------------------- decoders
def decode_configs(n):
    if n <= 65537:
        return [(w, avg) for w in (1, 2, 3, 8) for avg in (True, False)]
    return [(1, True), (3, True)]


@functools.lru_cache(maxsize=4)
def payload_codes(n, world):
    c = np.random.default_rng(n % 991 + world).integers(0, 256, world * n).astype(np.uint8)
    edge = np.array([0x00, 0x80, 0x7F, 0xFF, 0x01, 0x81], dtype=np.uint8)
    c[:min(edge.size, c.size)] = edge[:c.size]
    return c


@functools.lru_cache(maxsize=4)
def payload_halves(n, world):
    h = np.random.default_rng(n % 983 + world).integers(0, 1 << 16, world * n).astype(np.uint16)
    edge = np.array([0x0000, 0x8000, 0x0001, 0x7BFF, 0x7C00, 0xFC00, 0x7E00, 0x03FF], dtype=np.uint16)
    h[-min(edge.size, h.size):] = edge[:h.size]
    return h


@pytest.mark.parametrize("n,off", cases())
def test_natural_decompress(n, off):
    for world, avg in decode_configs(n):
        divisor = float(world) if avg else 1.0
        codes = payload_codes(n, world)
        c = Slot(world * n, U8, off, codes)
        for flavour in (0, 1):
            o = Slot(n, BF16, off)
            _lib.call("grace_natural_decompress_bf16", c.t.data_ptr(), n, world, n, flavour, 1, divisor, o.t.data_ptr(),
                      ops._stream())
            ref = ops.natural_decompress(c.t, n, flavour, world=world, aggregate=True, divisor=divisor)
            msg = U.same_bf16(o.bits(), torch_round(ref))
            assert msg is None and o.guards_intact(), (world, avg, flavour, msg)
            if n <= 4099:   # the numpy restatement as well
                want = U.natural_result(codes.reshape(world, n), flavour, divisor)
                assert U.same_bf16(o.bits(), want) is None, (world, avg, flavour)
        assert c.guards_intact() and np.array_equal(c.bits(), codes)
    if off == 0:
        out = ops.natural_decompress(c.t, n, 1, world=world, aggregate=True, divisor=divisor, out_dtype=BF16)
        assert out.dtype == BF16 and U.same_bf16(torch_round(out.float()), o.bits()) is None
        # aggregate off: the single payload's decode itself (-0 stays -0)
        one = ops.natural_decompress(c.t[:n], n, 0, out_dtype=BF16)
        assert U.same_bf16(torch_round(one.float()), U.narrow(O.natural_decode(codes[:n]))) is None


@pytest.mark.parametrize("n,off", cases())
def test_fp16_decompress_aggregate(n, off):
    for world, avg in decode_configs(n):
        divisor = float(world) if avg else 1.0
        halves = payload_halves(n, world)
        h = Slot(world * n, F16, off, halves)
        o = Slot(n, BF16, off)
        _lib.call("grace_fp16_decompress_aggregate_bf16", h.t.data_ptr(), n, world, n, divisor, o.t.data_ptr(),
                  ops._stream())
        ref = ops.fp16_decompress_aggregate(h.t, n, world, divisor=divisor)
        msg = U.same_bf16(o.bits(), torch_round(ref))
        assert msg is None and o.guards_intact(), (world, avg, msg)
        if n <= 4099:
            want = U.fp16_result(halves.view(np.float16).reshape(world, n), divisor)
            assert U.same_bf16(o.bits(), want) is None, (world, avg)
        assert h.guards_intact() and np.array_equal(h.bits(), halves)
    if off == 0:
        out = ops.fp16_decompress_aggregate(h.t, n, world, divisor=divisor, out_dtype=BF16)
        assert out.dtype == BF16 and U.same_bf16(torch_round(out.float()), o.bits()) is None


# ----------------------------------------------------------------------------- the f32 paths this touches
def test_f32_natural_code_of_a_nan_is_the_oracles():
    """natural_code's exponent round-up wraps for a NaN as the reference's int32 does: with a random int
    below its mantissa the code is 0 / 128 (it was the clamp's upper end, 127 / 255, while the add was
    signed), with one above it the exponent 255 clamps to 127 / 255.  Both f32 kernels that inline it."""
    x = np.array([np.nan, -np.nan, 1.5, np.nan, -np.nan, np.inf, -0.75, np.nan], dtype=np.float32)
    x[[0, 3]] = np.array([0x7FC00000, 0x7F800001], dtype=np.uint32).view(np.float32)
    x[[1, 4]] = np.array([0xFFC00000, 0xFFFFFFFF], dtype=np.uint32).view(np.float32)
    ri = np.array([0, 0x7FFFFE, 0, 0, 0, 0, 0, 0x3FFFFF], dtype=np.int32)
    want = O.natural_compress(x, ri)
    assert want.tolist()[:2] == [0, 255] and want.tolist()[3:5] == [0, 128]
    for n in (8, 5, 1):                                   # the quad path and the guarded tail
        got = ops.natural_compress(torch.from_numpy(x[:n].copy()).to(DEV), rand_int=torch.from_numpy(ri[:n].copy()).to(DEV))
        assert np.array_equal(got.cpu().numpy(), want[:n]), n
    # the fused f32 step decodes the separate encode's codes, NaNs included, under the same seed
    big = np.tile(x, 515)[:4099].copy()
    xf = torch.from_numpy(big).to(DEV)
    for seed in (1, 2, 3):
        codes = ops.natural_compress(xf, seed=seed)
        want_step = np.float32(0) + O.natural_decode(codes.cpu().numpy())
        got_step = ops.cast_step_w1(xf, 0, seed).cpu().numpy()
        assert np.array_equal(got_step.view(np.uint32), want_step.view(np.uint32)), seed
        c = codes.cpu().numpy()[np.isnan(big)]
        assert set(c.tolist()) <= {0, 128, 127, 255} and {0, 128} & set(c.tolist())       # some NaN rounded up


@pytest.mark.parametrize("codec", ["fp16", "natural", "cnat"])
def test_sharded_quant_encodes_a_bf16_shard_like_its_f32_values(codec):
    """grace_amd.dist's ShardedQuant has no dtype check beyond the ops encoders', which now take bf16: a
    bf16 shard is encoded as it is -- the codes of the widened values -- and the dense result stays
    f32, equal to the result for shard.float().  (No bf16 dense result: not on the bf16 path.)"""
    from grace_amd.dist.sharded_quant import ShardedQuant
    bits = grad_bits(4099, 4)
    g = torch.from_numpy(bits.view(np.int16).copy()).view(BF16).to(DEV)
    for dense in ("replicated", "shard"):
        a, b = ShardedQuant(codec, dense=dense, seed=11), ShardedQuant(codec, dense=dense, seed=11)
        out, ref = a.step(g), b.step(g.float())
        assert out.dtype == F32 and out.shape == ref.shape == (4099,)
        assert torch.equal(a.last_codes.view(torch.uint8), b.last_codes.view(torch.uint8))
        nan = torch.isnan(ref)
        assert torch.equal(torch.isnan(out), nan) and torch.equal(out[~nan].view(I32), ref[~nan].view(I32))
