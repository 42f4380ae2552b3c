"""One EF-signSGD step given the mean, and the world-W decode, restated in numpy from the oracle's
functions alone (oracle.grace_oracle: efsign_compensate, sign_encode, efsign_decode,
residual_update, python_sum).

The fused device step (grace_amd/csrc/sign.hip) computes its own mean -- another summation order
than torch's, held to 2 ulp -- and everything after the mean is exact given that mean.  So the
expected values of a device step are these functions with the device's mean injected.
tests/test_sign_bf16_util.py pins them to the reference's golden sequence."""
import numpy as np

from oracle import grace_oracle as O

F32 = np.float32


def ef_step(g, residual, lr_mem, mean, lr_agg=None):
    """(t, codes, dec, r', dense) of one rank's step: g f32 (a bf16 gradient widened), residual f32
    or None on a name's first step, `mean` the f32 mean to use.  dense = (0 + dec) / lr_agg, the
    world-1 result in f32 before any narrowing (None when lr_agg is None)."""
    t = O.efsign_compensate(g, residual, lr_mem).ravel()
    codes = O.sign_encode(t)
    with np.errstate(invalid="ignore", over="ignore"):
        dec = O.efsign_decode(np.asarray(mean, dtype=F32), codes)
        res = O.residual_update(t, dec)
        dense = None if lr_agg is None else (O.python_sum([dec]) / F32(lr_agg)).astype(F32)
    return t, codes, dec, res, dense


def exact_mean(t):
    """F32(F32(fsum|t|) / F32(n)): the bar the device mean is held to (2 ulp)."""
    import math
    a = np.abs(np.asarray(t, dtype=np.float64).ravel())
    if not np.isfinite(a).all():
        s = np.float64(np.nan) if np.isnan(a).any() else np.float64(np.inf)
    else:
        s = math.fsum(a.tolist())
    with np.errstate(over="ignore"):
        return F32(F32(s) / F32(a.size))


def ef_decode_aggregate(means, codes_wn, world, n, lr_agg):
    """(((0 + m_0 d_0) + m_1 d_1) + ...) / lr_agg in f32 over `world` payloads (codes rank-major)."""
    means = np.asarray(means, dtype=F32).ravel()
    codes_wn = np.asarray(codes_wn, dtype=np.uint8).reshape(world, n)
    with np.errstate(invalid="ignore", over="ignore"):
        decs = [O.efsign_decode(means[w:w + 1], codes_wn[w]) for w in range(world)]
        return (O.python_sum(decs) / F32(lr_agg)).astype(F32)


def same_bits_nan(a, b):
    """Bitwise equality of two f32 arrays except at NaNs, where only NaN-ness must agree (the sign
    and payload bits of a NaN that arithmetic produced differ between the host and the device)."""
    a, b = np.ascontiguousarray(a, dtype=F32).ravel(), np.ascontiguousarray(b, dtype=F32).ravel()
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb]))
