"""The 8-bit codebook quantiser of grace_amd/csrc/u8bit.hip against a numpy reference
of include/grace_hip_u8bit.h's arithmetic: np.float32 division, searchsorted over the edges, one f32
multiply, a sequential f32 sum.  Everything is compared bit for bit."""
import functools

import numpy as np
import pytest
import torch

from grace_amd import ops
from grace_amd.dist.communicator.allgather import Allgather
from grace_amd.dist.memory.none import NoneMemory
from grace_amd.u8bit import U8bitCompressor, grace_from_params

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
f32 = np.float32


def ref_encode(x, block, edges):
    """(codes i8[n], scales f32[nblk]) of the f32 array x"""
    n = x.size
    B = block or n
    nblk = -(-n // B)
    X = np.zeros(nblk * B, f32)
    X[:n] = x
    X = X.reshape(nblk, B)
    A = np.abs(X)
    a = np.where(np.isnan(A), f32(0), A).max(axis=1)
    with np.errstate(all="ignore"):
        y = A / a[:, None]
    i = np.clip(np.searchsorted(edges, y.reshape(-1), side="right") - 1, 0, None).reshape(y.shape)
    i = np.where(np.isnan(y), 0, i)
    return np.where(X < 0, -i, i).astype(np.int8).reshape(-1)[:n], a


def ref_decode(codes, scales, block, values):
    a = np.repeat(scales, block or codes.size)[:codes.size]
    with np.errstate(all="ignore"):
        mag = values[np.abs(codes.astype(np.int32))] * a
    return np.where(codes == 0, f32(0), np.where(codes < 0, -mag, mag)).astype(f32)


@functools.lru_cache(None)
def tables(kind):
    if kind == "user":
        v = np.sort(np.random.default_rng(5).random(128)).astype(f32)
        assert (np.diff(v) > 0).all()
        e, v = ops.u8bit_tables("nearest", v.tolist())
    else:
        e, v = ops.u8bit_tables(kind)
    return e, v, e.cpu().numpy(), v.cpu().numpy()


@functools.lru_cache(None)
def gradient(n, dtype):
    """randn scaled per 1000-element stretch by 1e-6 .. 1e3: (device tensor, its values as f32 numpy)"""
    g = torch.Generator().manual_seed(n)
    x = torch.randn(n + 1, generator=g) * 10.0 ** ((torch.arange(n + 1) // 1000 % 10) - 6).float()
    x = x.to(dtype)
    return x.to(DEV), x.float().numpy()


def bits(t):
    t = t.detach().cpu().contiguous().reshape(-1)
    return t.view(torch.int16 if t.dtype == BF16 else torch.int32).numpy()


def check(xd, x, block, kind):
    edges, values, e_np, v_np = tables(kind)
    codes, scales = ref_encode(x, block, e_np)
    got_c, got_s = ops.u8bit_compress(xd, block, edges)
    assert np.array_equal(got_c.cpu().numpy(), codes)
    assert np.array_equal(bits(got_s), scales.view(np.int32))
    got_s, out = ops.u8bit_step_w1(xd, block, edges, values)
    assert out.dtype == xd.dtype and out.shape == xd.shape
    assert np.array_equal(bits(got_s), scales.view(np.int32))
    want = torch.from_numpy(f32(0) + ref_decode(codes, scales, block, v_np)).to(xd.dtype)
    assert np.array_equal(bits(out), bits(want))
    return codes


@pytest.mark.parametrize("kind", ["floor", "nearest", "user"])
@pytest.mark.parametrize("n", [1, 255, 4097, 3 * 4096 + 17, (1 << 20) + 3])
@pytest.mark.parametrize("block", [0, 256, 512, 4096])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_compress_and_step(dtype, block, n, kind):
    xd, x = gradient(n, dtype)
    codes = check(xd[:n], x[:n], block, kind)
    if n > 100000 and block == 256:
        assert len(np.unique(np.abs(codes))) == 128     # the inputs reach every level


@pytest.mark.parametrize("block", [0, 256, 4096])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_pointer_off_the_16_byte_grid(dtype, block):
    xd, x = gradient(3 * 4096 + 17, dtype)
    assert xd.data_ptr() % 16 == 0
    check(xd[1:], x[1:], block, "floor")


@pytest.mark.parametrize("block", [0, 256])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_special_values(dtype, block):
    e_np = tables("floor")[2]
    x = gradient(4096 + 5, F32)[1][:4096 + 5].copy()
    x[0:256] = 0.0                                   # a whole block of zeros, one of them negative
    x[7] = -0.0
    x[300] = np.nan                                  # a block with a NaN
    x[600], x[601] = np.inf, -np.inf                 # a block with both infinities
    x[768:1024] = np.random.default_rng(1).uniform(-3, 3, 256)
    x[770] = -4.0                                    # the block's maximum, negative: code -127
    x[800:928] = e_np * f32(4.0)                     # y on every edge exactly
    x[928:1024:2] *= -1
    xt = torch.from_numpy(x).to(dtype)
    codes = check(xt.to(DEV), xt.float().numpy(), block, "floor")
    if block and dtype == F32:
        assert codes[770] == -127 and np.array_equal(codes[800:928], np.arange(128))
        assert not codes[:256].any() and codes[300] == 0


@pytest.mark.parametrize("out_dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("averaged", [False, True])
@pytest.mark.parametrize("block", [0, 512])
@pytest.mark.parametrize("n", [255, 2 * 4096 + 8, 2 * 4096 + 9])      # + 8: the packed loads at W > 1
@pytest.mark.parametrize("world", [1, 3])
def test_decode_aggregate(world, n, block, averaged, out_dtype):
    values, v_np = tables("nearest")[1], tables("nearest")[3]
    rng = np.random.default_rng(n + world)
    nblk = -(-n // block) if block else 1
    codes = rng.integers(-127, 128, (world, n)).astype(np.int8)
    codes[:, ::17] = 0
    scales = rng.uniform(1e-3, 10.0, (world, nblk)).astype(f32)
    divisor = world if averaged else 1
    acc = np.zeros(n, f32)
    for w in range(world):
        acc = acc + ref_decode(codes[w], scales[w], block, v_np)
    if divisor != 1:
        acc = acc / f32(divisor)
    got = ops.u8bit_decode_aggregate(torch.from_numpy(codes).reshape(-1).to(DEV),
                                     torch.from_numpy(scales).reshape(-1).to(DEV), world, n, block, values,
                                     divisor=divisor, out_dtype=out_dtype)
    assert got.dtype == out_dtype
    assert np.array_equal(bits(got), bits(torch.from_numpy(acc).to(out_dtype)))


@pytest.mark.parametrize("block", [0, 1024])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_allgather_step_is_the_fused_step(dtype, block):
    xd = gradient(4097, dtype)[0][:4096].view(64, 64)
    edges, values = tables("floor")[:2]
    out = Allgather(U8bitCompressor(block), NoneMemory(), 1).step(xd, "w")
    assert out.dtype == dtype and out.shape == xd.shape
    assert np.array_equal(bits(out), bits(ops.u8bit_step_w1(xd, block, edges, values)[1]))


def test_decode_aggregate_gathered_equals_the_decompress_loop():
    comp = U8bitCompressor(256, rounding="nearest")
    xs = [gradient(n, F32)[0][:4097] for n in (4097, 3 * 4096 + 17, (1 << 20) + 3)]
    pay = [comp.compress(x, "w") for x in xs]
    ctx = pay[0][1]
    gathered = [torch.cat([p[0][j] for p in pay]) for j in range(2)]
    got = comp.decode_aggregate_gathered(gathered, ctx, 3)
    want = np.zeros(4097, f32)
    for p, _ in pay:
        want = want + comp.decompress(p, ctx).cpu().numpy()
    assert np.array_equal(bits(got), (want / f32(3)).view(np.int32))


def test_grace_from_params_builds_and_steps():
    comm = grace_from_params({'compressor': 'u8bit', 'memory': 'none', 'communicator': 'allgather', 'world_size': 1,
                              'block_size': 256})
    assert isinstance(comm.compressor, U8bitCompressor) and comm.compressor.block_size == 256
    xd = gradient(4097, F32)[0][:4097]
    out = comm.step(xd, "w")
    e, v = tables("floor")[:2]
    assert np.array_equal(bits(out), bits(ops.u8bit_step_w1(xd, 256, e, v)[1]))
