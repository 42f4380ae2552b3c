"""tests/cast_bf16_util.py against torch's CPU casts and the oracle: the two bf16 conversions on ties,
±0, denormals, inf and NaN, the special-value tables the GPU tests plant, and one-bit's formulas."""
import numpy as np
import torch

from oracle import grace_oracle as O
from tests import cast_bf16_util as U

F32 = np.float32


def _torch_narrow(x):
    return torch.from_numpy(np.array(x, dtype=F32)).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)


def _torch_widen(bits):
    return torch.from_numpy(np.array(bits, dtype=np.uint16).view(np.int16)).view(torch.bfloat16).float().numpy()


def test_widen_is_torchs_cast_on_every_pattern():
    bits = np.arange(1 << 16, dtype=np.uint16)
    got, want = U.widen(bits), _torch_widen(bits)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(U.narrow(got)[~np.isnan(got)], bits[~np.isnan(got)])      # the round trip is exact


def test_narrow_is_torchs_cast_on_ties_zeros_denormals_inf_and_nan():
    rng = np.random.default_rng(5)
    hi = rng.integers(0, 1 << 16, 4096).astype(np.uint32) << 16
    cases = [hi | 0x8000, hi | 0x7FFF, hi | 0x8001, hi | rng.integers(0, 1 << 16, 4096).astype(np.uint32)]   # ties first
    cases.append(np.array([0x00000000, 0x80000000, 0x00000001, 0x00008000, 0x00018000, 0x007FFFFF, 0x807FFFFF,
                           0x7F7FFFFF, 0x7F800000, 0xFF800000, 0x7F7F8000, 0x7F7F7FFF], dtype=np.uint32))
    x = np.concatenate(cases).view(F32)
    got, want = U.narrow(x), _torch_narrow(x)
    nan = np.isnan(x)
    assert np.array_equal(got[~nan], want[~nan])
    assert (got[nan] == 0x7FC0).all() and np.isnan(U.widen(want[nan])).all()
    nans = np.array([0x7FC00000, 0xFFC00001, 0x7F800001, 0x7FFFFFFF], dtype=np.uint32).view(F32)
    assert (U.narrow(nans) == 0x7FC0).all()
    # a tie goes to the even pattern, a denormal is rounded, not flushed
    assert U.narrow(np.array([0x3F808000, 0x3F818000, 0x00008000, 0x00018000], dtype=np.uint32).view(F32)).tolist() == \
        [0x3F80, 0x3F82, 0x0000, 0x0002]


def test_special_tables_are_bf16_representable_and_do_what_the_tests_say():
    for table in (U.SPECIALS, U.FP16_EDGES, U.NATURAL_EDGES):
        keep = ~np.isnan(table)
        assert np.array_equal(U.representable(table)[keep].view(np.uint32), table[keep].view(np.uint32))
    bits = U.narrow(U.SPECIALS)
    assert {0x0000, 0x8000, 0x0001, 0x8001, 0x0060, 0x7F80, 0xFF80, 0x7FC0} == set(bits.tolist())
    with np.errstate(all="ignore"):
        h = O.fp16_compress(U.FP16_EDGES).view(np.uint16).tolist()
    assert h == [0x7BF8, 0x7C00, 0x0400, 0x0001, 0x0000, 0x0001]
    # the natural codes clip at biased exponents 18 and 145: 2^-110 (17) and 2^-109 (18) share code 0
    # with no round-up, 2^20 (147) saturates
    zero = np.zeros(U.NATURAL_EDGES.size, dtype=np.int32)
    assert O.natural_compress(U.NATURAL_EDGES, zero + 0x7FFFFF).tolist() == [0, 0, 127, 128, 255]
    # cnat's table is one exponent step off: biased 17 -> 0, 18 -> 1
    assert O.cnat_compress(U.NATURAL_EDGES).tolist() == [0, 1, 127, 128, 255]


def test_cast_step_is_decode_of_encode_rounded_once():
    x = U.representable(np.concatenate([np.random.default_rng(1).standard_normal(64).astype(F32), U.FP16_EDGES]))
    bits = U.narrow(x)
    with np.errstate(over="ignore"):
        want = _torch_narrow(np.float32(0) + x.astype(np.float16).astype(F32))
    assert U.same_bf16(U.cast_step(bits, 3), want) is None
    ri = np.full(x.size, 0x7FFFFF, dtype=np.int32)      # never round up: the exponent alone survives
    got = U.widen(U.cast_step(bits, 0, ri))
    assert np.array_equal(got, O.natural_decode(O.natural_compress(x, ri)) + F32(0))
    assert U.same_bf16(U.cast_step(bits, 2), U.narrow(F32(0) + O.cnat_decode(O.cnat_compress(x)))) is None


def test_same_bf16_reports_bits_and_nan_positions():
    a = np.array([0x3F80, 0x7FC0, 0x0000], dtype=np.uint16)
    assert U.same_bf16(a, a) is None
    assert U.same_bf16(np.array([0x3F80, 0xFFC1, 0x0000], dtype=np.uint16), a) is None      # NaN-ness only
    assert "first at 2" in U.same_bf16(np.array([0x3F80, 0x7FC0, 0x8000], dtype=np.uint16), a)
    assert "first at 1" in U.same_bf16(np.array([0x3F80, 0x3F80, 0x0000], dtype=np.uint16), a)


def test_onebit_formulas_are_the_oracles():
    rng = np.random.default_rng(2)
    for x in (U.representable(rng.standard_normal(1000).astype(F32)), np.array([1.5, 2.5], dtype=F32),
              np.array([-1.5, -0.5], dtype=F32), np.array([0.0, -0.0], dtype=F32), np.array([-3.0], dtype=F32)):
        mask, m0, m1 = O.onebit_compress(x)
        assert np.array_equal(U.onebit_mask(x), mask)
        g0, g1 = U.onebit_fin(*U.onebit_exact_sums(x), x.size)
        assert U.ulps_apart(g0, m0) <= 4 and U.ulps_apart(g1, m1) <= 4       # torch sums in f32 cascades
        for quirk in (False, True):
            assert np.array_equal(U.onebit_dec(mask, m0, m1, quirk), O.onebit_decode(mask, m0, m1, quirk=quirk))
    # an empty class keeps its sum (0) as its mean; NaN is "not x < 0"; inf * 0 is NaN in the decode
    assert U.onebit_fin(0.0, 0.0, 4.0, 2) == (F32(0), F32(2))
    assert U.onebit_mask(np.array([np.nan, -np.nan, -1.0, -0.0], dtype=F32)).tolist() == [0, 0, 1, 0]
    s0, n0, s1 = U.onebit_exact_sums(np.array([-1.0, np.inf, 2.0], dtype=F32))
    assert (s0, n0, s1) == (-1.0, 1.0, np.inf)
    d = U.onebit_dec(np.array([1, 0], dtype=np.uint8), F32(-1), F32(np.inf), False)
    assert np.isnan(d[0]) and d[1] == np.inf
    assert U.ulps_apart(F32(1.0), np.nextafter(F32(1.0), F32(2.0))) == 1
    assert U.ulps_apart(F32(-0.0), F32(0.0)) == 0 and U.ulps_apart(F32(1.0), F32(np.nan)) > 2
