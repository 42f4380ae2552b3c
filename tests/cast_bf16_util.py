"""numpy restatement of what grace_amd/csrc/cast.hip computes on a bfloat16 gradient:
the oracle's functions on the widened gradient, one round-to-nearest-even to bf16 at the end, and
one-bit's means formula and decode.  A bf16 array is its 16-bit patterns, np.uint16.
tests/test_cast_bf16_util.py checks the two conversions against torch's CPU casts."""
import math

import numpy as np

from oracle import grace_oracle as O

F32 = np.float32
U16 = np.uint16
# ±0, bf16 denormals (smallest, largest), ±inf, NaN -- as f32 values that bf16 holds exactly
SPECIALS = np.array([0.0, -0.0, 2.0 ** -133, -(2.0 ** -133), 2.0 ** -127 + 2.0 ** -128, np.inf, -np.inf, np.nan],
                    dtype=np.float64).astype(F32)
# the f16 range edges: the largest bf16 below the f16 overflow tie, 2^16 (-> inf), the smallest f16
# normal, the smallest f16 denormal, the tie 2^-25 (-> 0) and the bf16 just above it (-> 2^-24)
FP16_EDGES = np.array([65280.0, 65536.0, 2.0 ** -14, 2.0 ** -24, 2.0 ** -25, 2.0 ** -25 * (1 + 2.0 ** -7)], dtype=F32)
# exponents at both clip ends of the natural codecs
NATURAL_EDGES = np.array([2.0 ** -110, 2.0 ** -109, 2.0 ** 20, -(2.0 ** -110), -(2.0 ** 20)], dtype=F32)


def widen(bits):
    """bf16 patterns -> the f32 values they denote (exact)."""
    return (np.asarray(bits, dtype=U16).astype(np.uint32) << 16).view(F32)


def narrow(x):
    """f32 -> bf16 patterns, round to nearest even in integer arithmetic (subnormals are rounded,
    not flushed); a NaN becomes the quiet NaN 0x7FC0 (common.h f32_to_bf16)."""
    u = np.ascontiguousarray(x, dtype=F32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(U16)
    return np.where((u & 0x7FFFFFFF) > 0x7F800000, U16(0x7FC0), r).astype(U16)


def representable(x):
    """f32 values truncated to ones bf16 holds exactly (the low 16 bits cleared)."""
    return (np.ascontiguousarray(x, dtype=F32).view(np.uint32) & np.uint32(0xFFFF0000)).view(F32)


def same_bf16(got, want):
    """Equal 16-bit patterns; at a NaN of `want` only NaN-ness is compared.  Returns the first
    mismatch as a message, or None."""
    got, want = np.asarray(got, dtype=U16).ravel(), np.asarray(want, dtype=U16).ravel()
    if got.shape != want.shape:
        return f"shapes {got.shape} != {want.shape}"
    gn, wn = np.isnan(widen(got)), np.isnan(widen(want))
    bad = np.flatnonzero((gn != wn) | ((got != want) & ~wn))
    if bad.size:
        i = int(bad[0])
        return f"{bad.size} differ, first at {i}: got {int(got[i]):#06x}, want {int(want[i]):#06x}"
    return None


# ----------------------------------------------------------------------------- codes and results
def decode(codes, flavour):
    return O.natural_decode(codes) if flavour == 0 else O.cnat_decode(codes)


def aggregate(decoded, divisor):
    """((0 + d_0) + d_1 + ...) / divisor in f32, no division when divisor == 1, then one rounding."""
    with np.errstate(all="ignore"):
        acc = O.python_sum(decoded)
        if divisor != 1:
            acc = (acc / F32(divisor)).astype(F32)
    return narrow(acc)


def natural_result(codes_w, flavour, divisor):
    return aggregate([decode(c, flavour) for c in codes_w], divisor)


def fp16_result(halves_w, divisor):
    return aggregate([O.fp16_decode(h) for h in halves_w], divisor)


def cast_step(bits, mode, rand=None):
    """grace_cast_step_w1_bf16 given the randoms the device drew (natural: i32, cnat: f32)."""
    x = widen(bits)
    with np.errstate(all="ignore"):
        if mode == 0:
            d = O.natural_decode(O.natural_compress(x, rand))
        elif mode in (1, 2):
            d = O.cnat_decode(O.cnat_compress(x, None if mode == 2 else rand))
        else:
            d = O.fp16_decode(O.fp16_compress(x))
    return narrow(O.python_sum([d]))


# ----------------------------------------------------------------------------- one-bit
def onebit_mask(x):
    return (np.asarray(x, dtype=F32) < 0).astype(np.uint8)     # NaN: not x < 0


def onebit_exact_sums(x):
    """(S0, N0, S1): math.fsum over the f64-widened classes (exactly rounded to f64)."""
    x = np.asarray(x, dtype=F32).ravel()
    neg = x < 0
    s = []
    for part in (x[neg], x[~neg]):
        part = part.astype(np.float64)
        if np.isnan(part).any():
            s.append(float("nan"))
        elif np.isinf(part).any():
            s.append(float(np.sum(part[np.isinf(part)])))          # +inf, -inf, or nan for both
        else:
            s.append(math.fsum(part.tolist()))
    return s[0], float(np.count_nonzero(neg)), s[1]


def onebit_fin(s0, n0, s1, n):
    """OneBitFin's f32 formula (codec.h onebit_means) on three f64 sums."""
    with np.errstate(all="ignore"):
        sum0, num0, sum1 = F32(s0), F32(n0), F32(s1)
        num1 = F32(F32(n) - num0)
        mean0 = F32(sum0 / num0) if num0 > 0 else sum0
        mean1 = F32(sum1 / num1) if num1 > 0 else sum1
    return F32(mean0), F32(mean1)


def onebit_dec(mask0, mean0, mean1, quirk):
    """codec.h onebit_dec: two products, then the add (0 * inf is NaN)."""
    with np.errstate(all="ignore"):
        return O.onebit_decode(np.asarray(mask0, dtype=np.uint8), F32(mean0), F32(mean1), quirk=quirk)


def ulps_apart(a, b):
    """Distance in f32 ulps between two finite floats of one sign (or equal bits / both NaN: 0)."""
    a, b = F32(a), F32(b)
    if (np.isnan(a) and np.isnan(b)) or a.view(np.uint32) == b.view(np.uint32):
        return 0
    if np.isnan(a) or np.isnan(b) or np.isinf(a) or np.isinf(b):
        return 1 << 31
    key = lambda v: int(v.view(np.int32)) if v.view(np.int32) >= 0 else -int(v.view(np.int32) & 0x7FFFFFFF)
    return abs(key(a) - key(b))
