"""CPU self-test of tests/payload_bf16_util.py: the conversion payload really meets every rounding
decision, and the multi-rank cases tell a decode that rounds early from one that rounds once."""
import numpy as np
import torch

from tests import payload_bf16_util as B
from tests import payload_util as U


def test_conversion_payload_covers_every_rounding_decision():
    ranks = B.conversion_case()
    (vals, idx), = ranks
    assert vals.size == idx.size == B.CONV_K == 393216 and np.unique(idx).size == idx.size
    assert B.CONV_N == 48 * U.CHUNK + 5
    assert np.setdiff1d(np.arange(B.CONV_N), idx).tolist() == sorted(B.CONV_HOLES)
    per_chunk = np.bincount(idx.astype(np.int64) >> U.CHUNK_LOG, minlength=49)
    assert per_chunk[:48].min() > 256 and 0 < per_chunk[48] < 5      # many rounds; a touched partial chunk
    touched, ref = U.ref_aggregate(ranks, B.CONV_N, 1)
    rb = U.bits(ref)
    fin = ~np.isnan(ref)
    # the f32 result that the epilogue narrows still holds all six lower halves on every upper half
    # that is no NaN (0 + v = v but for -0.0)
    for low in B.LOWS:
        assert np.count_nonzero((rb[fin] & 0xFFFF) == low) >= 65536 - 2 * 128 - 2, hex(low)
    bits, nan = B.expected_touched(ranks, B.CONV_N, 1)[1:]
    assert nan.any() and np.array_equal(nan, np.isnan(ref))
    assert (bits == 0x7F80).any() and (bits == 0xFF80).any()                      # +-inf
    sub = ((bits & 0x7F80) == 0) & ((bits & 0x007F) != 0)
    assert sub.any() and (sub & (bits >> 15 == 1)).any()                           # subnormals of both signs
    # both outcomes of a tie, and a carry into the exponent
    up = (bits[fin].astype(np.int64) - (rb[fin] >> 16).astype(np.int64)) == 1
    assert up.any() and (~up).any()
    tie = (rb & 0xFFFF) == 0x8000
    assert (up[tie[fin]]).any() and (~up[tie[fin]]).any()
    dense_bits, dense_nan = B.expected_dense(ranks, B.CONV_N, 1)
    assert dense_bits.size == B.CONV_N and not dense_bits[list(B.CONV_HOLES)].any()
    assert np.array_equal(dense_bits[touched], bits) and np.array_equal(dense_nan[touched], nan)


def test_narrow_is_torchs_cpu_cast():
    x = np.array([1.0, 1.00390625, 1.01171875, -0.0, np.inf, np.nan, 1e-40], dtype=np.float32)
    bits, nan = B.narrow(x)
    assert bits[:5].tolist() == [0x3F80, 0x3F80, 0x3F82, 0x8000, 0x7F80] and nan.tolist() == [False] * 5 + [True, False]
    assert np.array_equal(bits, torch.from_numpy(x).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16))


def test_rounding_early_is_told_from_rounding_once():
    """Narrowing every rank's values first, and narrowing the sum before the division, each change at
    least one element of a multi-rank case: a kernel that rounds early cannot pass."""
    for world, divisor in ((2, 2), (9, 3), (65, 65)):
        ranks = U.sorted_base_case(world)
        bits, nan = B.expected_dense(ranks, U.BASE_N, divisor)
        early, enan = B.expected_dense(B.narrowed_first(ranks), U.BASE_N, divisor)
        assert np.any((early != bits) & ~nan & ~enan), (world, divisor)
    for world in (1, 9):      # (a division by a power of two commutes with the rounding: divisor 3)
        ranks = U.sorted_base_case(world)
        bits, nan = B.expected_dense(ranks, U.BASE_N, 3)
        touched, acc = U.ref_aggregate(ranks, U.BASE_N, 1)
        s = torch.from_numpy(acc).to(torch.bfloat16).float().numpy()        # the sum, narrowed too soon
        wrong, _ = B.narrow((s / np.float32(3)).astype(np.float32))
        assert np.any((wrong != bits[touched]) & ~nan[touched]), world


def test_assert_bits_compares_nan_by_nan_ness_only():
    exp_bits = np.array([0x3F80, 0x7FC0, 0x0000], dtype=np.uint16)
    exp_nan = np.array([False, True, False])
    B.assert_bits(np.array([0x3F80, 0xFFC1, 0x0000], dtype=np.uint16), exp_bits, exp_nan)
    for bad in ([0x3F81, 0x7FC0, 0], [0x3F80, 0x7F80, 0], [0x3F80, 0x7FC0, 0x7FC0]):
        try:
            B.assert_bits(np.array(bad, dtype=np.uint16), exp_bits, exp_nan)
        except AssertionError:
            continue
        raise AssertionError(bad)
