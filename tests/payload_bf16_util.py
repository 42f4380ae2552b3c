"""Host side of the bfloat16 sparse-decode tests (tests/test_gpu_payload_bf16.py): the expected bf16
result of the rank-ordered aggregate and the payload that meets every rounding decision.

The expected dense bf16 values are always built the same way: payload_util.ref_aggregate's f32
result, made dense with +0.0 elsewhere, then torch's CPU ``.to(torch.bfloat16)``; they are compared
as 16-bit patterns, at NaN positions only NaN-ness (tests/test_gpu_topk_bf16.py::check_dense)."""
import functools

import numpy as np
import torch

from tests import payload_util as U

BF16 = torch.bfloat16
LOWS = (0x0000, 0x0001, 0x7FFF, 0x8000, 0x8001, 0xFFFF)   # the lower halves that decide a rounding
CONV_K = 65536 * len(LOWS)
CONV_N = CONV_K + 5     # 48 full chunks of 8192 and a 5-element last chunk
CONV_HOLES = (7, 3 * U.CHUNK + 1, 100000, 250001, CONV_N - 2)   # the five untouched elements


def narrow(f32):
    """f32 array -> (bf16 bits as uint16, NaN mask), rounded as torch's CPU cast rounds."""
    a = np.ascontiguousarray(f32, dtype=np.float32)
    b = torch.from_numpy(a).to(BF16)
    return b.view(torch.int16).numpy().view(np.uint16), np.isnan(a)


def expected_touched(ranks, n, divisor):
    """(touched indices, expected bf16 bits there, NaN mask there): every other element is +0.0."""
    touched, ref = U.ref_aggregate(ranks, n, divisor)
    bits, nan = narrow(ref)
    return touched, bits, nan


def expected_dense(ranks, n, divisor):
    """(bf16 bits uint16[n], NaN mask bool[n]) of the dense result."""
    touched, ref = U.ref_aggregate(ranks, n, divisor)
    dense = np.zeros(n, dtype=np.float32)     # +0.0
    dense[touched] = ref
    return narrow(dense)


def assert_bits(got, exp_bits, exp_nan, what=""):
    """got: uint16 bits; equal to exp_bits outside NaN positions, NaN exactly at exp_nan."""
    got = np.asarray(got).view(np.uint16).ravel()
    assert got.size == exp_bits.size, (what, got.size, exp_bits.size)
    got_nan = (got & 0x7FFF) > 0x7F80
    assert np.array_equal(got_nan, exp_nan), (what, "NaN positions", np.flatnonzero(got_nan != exp_nan)[:8])
    bad = np.flatnonzero((got != exp_bits) & ~exp_nan)
    assert bad.size == 0, (what, bad[:8], got[bad[:8]], exp_bits[bad[:8]])


@functools.lru_cache(maxsize=1)
def conversion_case():
    """One rank whose values are all 65,536 upper halves x the six deciding lower halves (the
    patterns of tests/test_gpu_topk_bf16.py::_conversion_cases, in that order) at distinct indices
    of CONV_N elements: every chunk holds far more than 256 entries, and the last chunk is partial."""
    hi = np.arange(65536, dtype=np.uint32) << 16
    u = (hi[:, None] | np.array(LOWS, dtype=np.uint32)[None, :]).ravel()
    assert u.size == CONV_K
    free = np.setdiff1d(np.arange(CONV_N, dtype=np.int64), np.array(CONV_HOLES, dtype=np.int64))
    idx = np.random.default_rng(393216).permutation(free).astype(np.int32)
    assert idx.size == CONV_K
    vals = u.view(np.float32).copy()
    vals.setflags(write=False)
    idx.setflags(write=False)
    return [(vals, idx)]


def narrowed_first(ranks):
    """The same payloads with every rank's values rounded to bf16 before anything is added."""
    out = []
    for v, i in ranks:
        b = torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).to(BF16).float().numpy()
        out.append((b, i))
    return out
