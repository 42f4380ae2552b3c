"""The bf16 twins of the small sign kernels (grace_amd/csrc/sign.hip) at the level of grace_amd.ops:
a bf16 tensor gives the codes, words and Signum momentum of its exact f32 upcast, and every dense
result is +-1 in bf16 (0x3F80 / 0xBF80)."""
import numpy as np
import pytest
import torch

from oracle import grace_oracle as O
from tests.test_gpu_efsign_fused import SIZES, _edges_untouched, _grad, _view
from tests.test_gpu_topk_bf16 import _np

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16 = torch.bfloat16
ONE, MINUS_ONE = 0x3F80, 0xBF80


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int16).numpy().ravel().view(np.uint16)


def _pm1_bits(codes):
    return np.where(np.asarray(codes).ravel() != 0, ONE, MINUS_ONE).astype(np.uint16)


def _words(codes):
    """bit i of word i // 32, LSB first, zero past n (the pack_bits layout)."""
    c = np.asarray(codes, dtype=np.uint8).ravel()
    pad = np.zeros((-c.size) % 32, dtype=np.uint8)
    return np.packbits(np.concatenate([c, pad]), bitorder="little").view(np.uint32).view(np.int32)


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "offset1"])
@pytest.mark.parametrize("kind", ["normal", "special"])
@pytest.mark.parametrize("n", SIZES)
def test_codes_words_and_step_of_bf16_equal_the_upcast(n, kind, offset):
    from grace_amd import ops
    b, up = _grad(n, kind, 2)            # step 2 of "special": +-0, denormals, +-inf and NaN
    xbuf, x = _view(n, BF16, offset, b)
    before = xbuf.clone()
    exp = O.sign_encode(up)
    cbuf = torch.full((n + offset + 1,), 7, dtype=torch.uint8, device=DEV)
    cview = cbuf[offset:offset + n]
    codes = ops.sign_encode(x, out=cview)
    assert codes is cview and np.array_equal(_np(codes), exp)
    assert (_np(cbuf[:offset]) == 7).all() and (_np(cbuf[offset + n:]) == 7).all()
    assert np.array_equal(_np(ops.sign_encode(x)), exp)
    words = ops.sign_encode_bits(x)
    assert words.dtype == torch.int32 and np.array_equal(_np(words), _words(exp))
    # the same words and codes from the f32 kernels on the upcast, on the device
    x32 = torch.from_numpy(up).to(DEV)
    assert torch.equal(words, ops.sign_encode_bits(x32)) and torch.equal(codes, ops.sign_encode(x32))
    for want_codes in (True, False):     # False with an aligned x: the all-loads-before-any-store kernel
        c, out = ops.sign_step_w1(x, want_codes=want_codes)
        assert out.dtype == BF16 and out.shape == x.shape and (c is None) == (not want_codes)
        assert np.array_equal(_bits(out), _pm1_bits(exp))
        if want_codes:
            assert np.array_equal(_np(c), exp)
    obuf, out = _view(n, BF16, offset)
    ops.launch_sign_step_w1(x, out)
    assert np.array_equal(_bits(out), _pm1_bits(exp)) and _edges_untouched(obuf, offset, n)
    assert torch.equal(xbuf.view(torch.int16), before.view(torch.int16)), "x was written"


def test_world1_step_over_every_bf16_bit_pattern():
    from grace_amd import ops
    x = torch.from_numpy(np.arange(65536, dtype=np.uint16).view(np.int16)).view(BF16)
    exp = _pm1_bits(x.float().numpy() >= 0)          # NaN -> -1, -0 -> +1
    xd = x.to(DEV)
    for want_codes in (True, False):
        c, out = ops.sign_step_w1(xd, want_codes=want_codes)
        got = _bits(out)
        assert set(np.unique(got)) <= {ONE, MINUS_ONE} and np.array_equal(got, exp)
        if want_codes:
            assert np.array_equal(_np(c), (exp == ONE).astype(np.uint8))
    out = torch.empty_like(xd)
    ops.launch_sign_step_w1(xd, out)
    assert np.array_equal(_bits(out), exp)
    assert np.array_equal(_np(ops.sign_encode(xd)), (exp == ONE).astype(np.uint8))
    assert np.array_equal(_np(ops.sign_encode_bits(xd)), _words(exp == ONE))


@pytest.mark.parametrize("n", [5, 4099, 4100, 65537, 262149, 1048580])
@pytest.mark.parametrize("world", [1, 2, 3, 8])
def test_majority_u8_and_bits_with_bf16_output(world, n):
    from grace_amd import ops
    rng = np.random.default_rng(17 * world + n % 1013)
    codes = (rng.random((world, n)) < 0.5).astype(np.uint8)
    exp = O.sign_aggregate([O.sign_decode(codes[w]) for w in range(world)])
    exp_bits = _pm1_bits(exp > 0)
    got = ops.sign_majority(torch.from_numpy(codes.ravel()).to(DEV), world, n, out_dtype=BF16)
    assert got.dtype == BF16 and got.shape == (n,) and np.array_equal(_bits(got), exp_bits)
    words = np.concatenate([_words(codes[w]) for w in range(world)])
    wd = torch.from_numpy(words).to(DEV)
    got = ops.sign_majority_bits(wd, world, n, out_dtype=BF16)
    assert got.dtype == BF16 and got.shape == (n,) and np.array_equal(_bits(got), exp_bits)
    # the default is still f32, and equal to the oracle's +-1.0
    assert np.array_equal(_np(ops.sign_majority_bits(wd, world, n)), exp)
    assert np.array_equal(_np(ops.sign_majority(torch.from_numpy(codes.ravel()).to(DEV), world, n)), exp)


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "offset1"])
@pytest.mark.parametrize("n", [5, 4099, 262149, (1 << 23) + 5])
def test_signum_three_steps_equal_the_f32_kernel_on_the_upcast(n, offset):
    from grace_amd import ops
    beta = 0.9
    mbuf, m = _view(n, torch.float32, offset)
    m32 = torch.empty(n, device=DEV)
    prev = None
    for s in range(3):
        b, up = _grad(n, "special" if s == 2 else "normal", s)
        _, g = _view(n, BF16, offset, b)
        codes = ops.signum_encode(g, m, s > 0, beta)
        codes32 = ops.signum_encode(torch.from_numpy(up).to(DEV), m32, s > 0, beta)
        assert torch.equal(codes, codes32), s
        assert torch.equal(m.view(torch.int32), m32.view(torch.int32)), f"step {s}: momentum"
        assert m.dtype == torch.float32 and _edges_untouched(mbuf, offset, n)
        prev = O.signum_momentum(up, prev, beta)
        keep = ~np.isnan(prev)
        assert np.array_equal(_np(m).view(np.uint32)[keep], prev.view(np.uint32)[keep]), f"step {s}: oracle momentum"
        assert np.array_equal(_np(codes), O.sign_encode(prev)), s
