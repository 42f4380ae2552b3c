"""The world > 1 sparse decode with a bfloat16 result: grace_sparse_aggregate_sorted_bf16
(payload.hip, chunk_accumulate_kernel with uint16_t output) through
ops.sparse_aggregate_sorted(..., out_dtype=torch.bfloat16), on host-grouped payloads.

Expected: tests/payload_util.ref_aggregate's f32 result, dense with +0.0 elsewhere, rounded once by
torch's CPU cast (tests/payload_bf16_util.py), as 16-bit patterns; NaN positions by NaN-ness."""
import numpy as np
import pytest
import torch

from grace_amd import _lib, ops
from tests import payload_bf16_util as B
from tests import payload_util as U

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16 = torch.bfloat16
CH = U.CHUNK
SENTINEL = 0x4140      # 12.0: the bits around an output view


def _dev(words):
    return torch.from_numpy(np.ascontiguousarray(words).view(np.float32)).to(DEV)


def _bits16(t):
    return t.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16).ravel()


def _divisors(world):
    return tuple(dict.fromkeys((world, 1, 3)))


def _check(out, ranks, n, divisor, what):
    assert out.dtype == BF16 and out.numel() == n
    B.assert_bits(_bits16(out), *B.expected_dense(ranks, n, divisor), what)


def _bf16_call(g, k, stride, world, divisor, out, n):
    ow = (k + 1) // 2
    _lib.call("grace_sparse_aggregate_sorted_bf16", g.data_ptr(), g[k:].data_ptr(), g[k + ow:].data_ptr(), stride,
              world, float(divisor), out.data_ptr(), n, ops._stream())


# ------------------------------------------------------------------------------- every rounding decision
def test_conversion_payload_is_the_step_tests_patterns():
    from tests.test_gpu_topk_bf16 import _conversion_cases
    assert np.array_equal(U.bits(B.conversion_case()[0][0]), _conversion_cases()[0].numpy().view(np.uint32))


@pytest.mark.parametrize("shift", [0, 1, 2, 4])
def test_every_rounding_decision(shift):
    """World 1, divisor 1: 65,536 upper halves x six lower halves through the epilogue, 48 full chunks
    with far more than 256 entries each and a 5-element last chunk.  shift 0: a new aligned result;
    1, 2, 4: a view that many elements (2, 4, 8 bytes) into a buffer, so the vector and the guarded
    store are both taken whatever the vector width; the elements around the view keep their bits."""
    ranks, n = B.conversion_case(), B.CONV_N
    k = ranks[0][1].size
    g = _dev(U.gathered_words(ranks, n))
    if shift == 0:
        out = ops.sparse_aggregate_sorted(g, k, 1, n, 1, out_dtype=BF16)
        assert out.data_ptr() % 16 == 0
    else:
        big = torch.full((n + 16,), SENTINEL, dtype=torch.int16, device=DEV).view(BF16)
        assert big.data_ptr() % 16 == 0
        out = big[shift:shift + n]
        assert out.data_ptr() % 16 == 2 * shift
        _bf16_call(g, k, ops.sorted_payload_len(k, n), 1, 1, out, n)
        rest = np.concatenate([_bits16(big[:shift]), _bits16(big[shift + n:])])
        assert rest.size == 16 and np.all(rest == SENTINEL), shift
    _check(out, ranks, n, 1, shift)


# ------------------------------------------------------------------------------- branches
@pytest.mark.parametrize("world", [1, 2, 8, 9, 64, 65, 257])
def test_bf16_aggregate_every_branch(world):
    """The f32 decode's launch branches (register and LDS bounds, a clamped second rank batch, rank
    counts around the 256-entry round, a partial last chunk), rounded once after sum and division."""
    n = U.BASE_N
    ranks = U.sorted_base_case(world)
    k = ranks[0][1].size
    g = _dev(U.gathered_words(ranks, n))
    for divisor in _divisors(world):
        _check(ops.sparse_aggregate_sorted(g, k, world, n, divisor, out_dtype=BF16), ranks, n, divisor,
               (world, divisor))


def test_bf16_aggregate_whole_last_chunk():
    world, n = 9, 6 * CH
    ranks = U.sorted_base_case(world, n)
    k = ranks[0][1].size
    g = _dev(U.gathered_words(ranks, n))
    for divisor in _divisors(world):
        _check(ops.sparse_aggregate_sorted(g, k, world, n, divisor, out_dtype=BF16), ranks, n, divisor, divisor)


# ------------------------------------------------------------------------------- size
def test_bf16_aggregate_large():
    """n = 2^26 + 2 * 8192 + 5 (more than 8192 output chunks), checked on the device at the touched
    indices, plus the count of non-zero 16-bit patterns."""
    world, n, k = U.SORTED_LARGE[0]
    assert n == (1 << 26) + 2 * CH + 5
    ranks = U.sorted_large_case(world, n, k)
    g = _dev(U.gathered_words(ranks, n))
    for divisor in (world, 1):
        out = ops.sparse_aggregate_sorted(g, k, world, n, divisor, out_dtype=BF16)
        touched, bits, nan = B.expected_touched(ranks, n, divisor)
        assert out.dtype == BF16 and out.numel() == n
        B.assert_bits(_bits16(out[torch.from_numpy(touched).to(DEV)]), bits, nan, divisor)
        assert int(torch.count_nonzero(out.view(torch.int16))) == int(np.count_nonzero(bits)), divisor
        del out


# ------------------------------------------------------------------------------- the interface
def test_out_dtype_float16_is_refused():
    ranks = U.sorted_base_case(2)
    k = ranks[0][1].size
    g = _dev(U.gathered_words(ranks, U.BASE_N))
    with pytest.raises(TypeError):
        ops.sparse_aggregate_sorted(g, k, 2, U.BASE_N, 2, out_dtype=torch.float16)


def test_f32_default_is_unchanged():
    world, n = 9, U.BASE_N
    ranks = U.sorted_base_case(world)
    k = ranks[0][1].size
    g = _dev(U.gathered_words(ranks, n))
    for out in (ops.sparse_aggregate_sorted(g, k, world, n, 3),
                ops.sparse_aggregate_sorted(g, k, world, n, 3, out_dtype=torch.float32)):
        assert out.dtype == torch.float32
        touched, ref = U.ref_aggregate(ranks, n, 3)
        exp = np.zeros(n, dtype=np.uint32)
        exp[touched] = U.bits(ref)
        assert np.array_equal(out.cpu().numpy().view(np.uint32), exp)
