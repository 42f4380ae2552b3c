"""tests/sign_bf16_util.py against the reference's golden EF-signSGD sequence: fed the golden means,
the restated step reproduces the golden t, codes, dec and residuals bit for bit, so the expected
values of the GPU tests are pinned before any GPU run."""
import numpy as np

from tests import sign_bf16_util as U
from tests.golden_util import same_bits


def test_ef_step_reproduces_the_golden_sequence(golden):
    c = golden.case("sign", "efsignsgd_seq")
    lr = c.meta["lr"]
    res, decs = None, []
    for s in range(c.meta["steps"]):
        t, codes, dec, res, dense = U.ef_step(c[f"x{s}"], res, lr, c[f"mean{s}"], lr_agg=lr)
        assert same_bits(t, c[f"t{s}"].ravel()), s
        assert np.array_equal(codes, c[f"codes{s}"].ravel()), s
        assert same_bits(dec, c[f"dec{s}"].ravel()), s
        assert same_bits(res, c[f"res{s}"].ravel()), s
        assert U.same_bits_nan(res, c[f"res{s}"])
        # the exactly summed mean is within the project's 2 ulp of torch's
        m, e = c[f"mean{s}"].reshape(()), U.exact_mean(t)
        assert abs(int(m.view(np.int32)) - int(e.view(np.int32))) <= 2, (s, m, e)
        # world 1: the decode of one payload is the step's own dense result
        assert same_bits(U.ef_decode_aggregate(c[f"mean{s}"], codes, 1, codes.size, lr), dense), s
        decs.append((c[f"mean{s}"], codes))
    # three payloads as three ranks: python_sum in rank order, then the division
    means = np.concatenate([m.ravel() for m, _ in decs])
    codes = np.concatenate([k for _, k in decs])
    got = U.ef_decode_aggregate(means, codes, 3, decs[0][1].size, lr)
    exp = ((np.float32(0) + c["dec0"].ravel()) + c["dec1"].ravel() + c["dec2"].ravel()) / np.float32(lr)
    assert same_bits(got, exp.astype(np.float32))


def test_same_bits_nan_and_exact_mean_edges():
    a = np.array([1.0, np.nan, -0.0], dtype=np.float32)
    b = a.copy()
    b.view(np.uint32)[1] ^= 0x80000001          # another NaN
    assert U.same_bits_nan(a, b)
    b[2] = 0.0
    assert not U.same_bits_nan(a, b)             # +0 is not -0
    assert not U.same_bits_nan(a, np.array([1.0, 2.0, -0.0], dtype=np.float32))
    assert np.isnan(U.exact_mean(np.array([1.0, np.nan, np.inf], dtype=np.float32)))
    assert np.isinf(U.exact_mean(np.array([1.0, -np.inf], dtype=np.float32)))
    assert U.exact_mean(np.array([1e-45, -1e-45, 0.0, 3.0], dtype=np.float32)) == np.float32(0.75)
