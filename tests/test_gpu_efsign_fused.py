"""The fused EF-signSGD step (grace_amd/csrc/sign.hip: ops.efsign_step, ops.efsign_decode_aggregate)
in both gradient dtypes.

The specification: codes are the oracle's; the mean is within 2 ulp of the
exactly summed F32(F32(fsum|t|) / F32(n)) and the same bits on every call; everything after the mean
-- the residual and the dense result -- is exact given the mean the device used, so it is compared
bit for bit with tests/sign_bf16_util.py fed that mean, and with the unfused device kernels
(axpby, sign_encode, sign_decode(scale=mean), sub, sum_rank_order, div_scalar) fed it too.  A bf16
result is the f32 one rounded once by torch's CPU cast (check_dense).  At a NaN only NaN-ness is
compared: the sign and payload of a NaN that arithmetic produced are free.

Inputs are bf16-representable, so the f32 and the bf16 runs take the same values.  "special" plants
+-0 and bf16 denormals at both ends and inside on every step, +-inf as well from the second step on
(the mean is then inf) and NaN on the third (the mean is NaN): planted all at once, the first
step's NaN mean would leave the two steps that have a residual nothing but NaNs to compare."""
import numpy as np
import pytest
import torch

from tests import sign_bf16_util as U
from tests.test_gpu_topk_bf16 import _np, check_dense

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16 = torch.bfloat16
F32 = torch.float32

# 1, 3, 5: no full quad / one quad and a tail; 4099: a few waves and a ragged end; 65,537 = 257 scalar-path
# workgroups; 262,149 and 1,048,579: the striding reductions of tests/test_gpu_elementwise.py's RED_SIZES;
# 2^23 + 5: one quad and a tail past the vector kernels' grid wrap (2048 workgroups x 256 lanes x 4 quads)
SIZES = [1, 3, 5, 4099, 65537, 262149, 1048579, (1 << 23) + 5]
SENT = 12288.0      # what the elements around a view hold (exact in bf16)


def _grad(n, kind, step):
    """(bf16 CPU tensor, its exact f32 upcast)."""
    rng = np.random.default_rng(1000 * step + n % 997 + (7 if kind == "special" else 0))
    x = rng.standard_normal(n).astype(np.float32)
    if kind == "special":
        plant = [0.0, -0.0, 1e-40, -1e-40, 9.2e-41]
        if step >= 1:
            plant += [np.inf, -np.inf]
        if step >= 2:
            plant += [np.nan]
        spots = sorted({0, n - 1, n // 2, n // 3, 1 % n, (n - 2) % n, 4097 % n, (n - 5) % n})
        for j, i in enumerate(spots):
            x[i] = plant[(j + step) % len(plant)]
        if n > 16:     # every planted value is somewhere, whatever the spots took
            x[5:5 + len(plant)] = plant
    b = torch.from_numpy(x).to(BF16)
    return b, b.float().numpy()


def _view(n, dtype, offset, src=None):
    """(the whole buffer, the n-element view at `offset`): the view holds src, the rest SENT."""
    buf = torch.full((n + offset + 1,), SENT, dtype=dtype, device=DEV)
    v = buf[offset:offset + n]
    if src is not None:
        v.copy_(src)
    return buf, v


def _edges_untouched(buf, offset, n):
    e = torch.cat([buf[:offset], buf[offset + n:]]).float().cpu().numpy()
    return bool((e == SENT).all())


def _ulps(a, b):
    a, b = np.float32(a), np.float32(b)
    if np.isnan(a) or np.isnan(b):
        return 0 if np.isnan(a) and np.isnan(b) else 1 << 31
    if np.isinf(a) or np.isinf(b):
        return 0 if a == b else 1 << 31
    return abs(int(a.view(np.int32)) - int(b.view(np.int32)))


def _unfused(g32, r, has, lr_mem, mean, lr_agg):
    """(t, codes, r', dense f32) from the unfused f32 device kernels, fed the mean."""
    from grace_amd import ops
    t = ops.axpby(r, g32, 1.0, lr_mem) if has else g32
    codes = ops.sign_encode(t)
    dec = ops.sign_decode(codes, scale=mean)
    return t, codes, ops.sub(t, dec), ops.div_scalar(ops.sum_rank_order([dec]), lr_agg)


@pytest.mark.parametrize("kind,lr_mem,lr_agg", [("normal", 0.1, 0.1), ("special", 0.05, 0.3)])
@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "offset1"])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("n", SIZES)
def test_three_steps_of_one_name(n, dtype, offset, kind, lr_mem, lr_agg):
    from grace_amd import ops
    rbuf, r = _view(n, F32, offset)
    res = None
    for s in range(3):
        b, up = _grad(n, kind, s)
        gbuf, g = _view(n, dtype, offset, b if dtype == BF16 else torch.from_numpy(up))
        g_before = gbuf.clone()
        obuf, out = _view(n, dtype, offset)
        has = s > 0
        # the same call on copies of the inputs first: the mean must come out with the same bits
        _, r2 = _view(n, F32, offset, r if has else None)
        r_before = r.clone()
        mean2, _, _ = ops.efsign_step(g, r2, has, lr_mem, lr_agg, want_codes=False)
        mean, codes, got_out = ops.efsign_step(g, r, has, lr_mem, lr_agg, want_codes=True, out=out)
        assert got_out is out and mean.dtype == F32 and mean.shape == (1,) and codes.dtype == torch.uint8
        m = _np(mean)
        assert _np(mean2).tobytes() == m.tobytes(), f"step {s}: the mean differs between two calls"
        assert torch.equal(gbuf.view(torch.int16 if dtype == BF16 else torch.int32),
                           g_before.view(torch.int16 if dtype == BF16 else torch.int32)), "g was written"
        assert _edges_untouched(rbuf, offset, n) and _edges_untouched(obuf, offset, n), s

        t, exp_codes, _, res_exp, dense = U.ef_step(up, res, lr_mem, m, lr_agg)
        exact = U.exact_mean(t)
        print(f"n={n} step={s} mean={m[0]!r} exact={exact!r} ulps={_ulps(m[0], exact)}")
        assert _ulps(m[0], exact) <= 2, (s, m[0], exact)
        assert np.array_equal(_np(codes), exp_codes), f"step {s}: codes"
        assert U.same_bits_nan(_np(r), res_exp), f"step {s}: residual"
        assert U.same_bits_nan(_np(r2), res_exp), f"step {s}: residual of the repeated call"
        if dtype == BF16:
            check_dense(out, dense)
        else:
            assert U.same_bits_nan(_np(out), dense), f"step {s}: dense result"

        # the unfused device kernels, fed the device's mean
        g32 = torch.from_numpy(up).to(DEV)
        t_d, codes_d, res_d, dense_d = _unfused(g32, r_before, has, lr_mem, mean, lr_agg)
        assert torch.equal(codes, codes_d), f"step {s}: codes against the unfused kernels"
        assert U.same_bits_nan(_np(r), _np(res_d)), f"step {s}: residual against the unfused kernels"
        if dtype == BF16:
            check_dense(out, _np(dense_d))
        else:
            assert U.same_bits_nan(_np(out), _np(dense_d)), f"step {s}: dense against the unfused kernels"
        res = res_exp


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_outputs_are_optional_and_the_first_step_ignores_the_buffer(dtype):
    """want_codes=False / out=None write neither; has_residual=False does not read the residual
    buffer (it holds NaNs here) and has no lr_mem factor."""
    from grace_amd import ops
    n = 4099
    b, up = _grad(n, "normal", 5)
    g = (b if dtype == BF16 else torch.from_numpy(up)).to(DEV)
    r = torch.full((n,), float("nan"), device=DEV)
    mean, codes, out = ops.efsign_step(g, r, False, 123.0, 0.5, want_codes=False)
    assert codes is None and out is None
    _, _, _, res_exp, dense = U.ef_step(up, None, 123.0, _np(mean), 0.5)
    assert U.same_bits_nan(_np(r), res_exp) and not np.isnan(_np(r)).any()
    out = torch.empty(n, dtype=dtype, device=DEV)
    r2 = torch.full((n,), float("nan"), device=DEV)
    mean2, codes, _ = ops.efsign_step(g, r2, False, 1.0, 0.5, want_codes=True, out=out)
    assert _np(mean2).tobytes() == _np(mean).tobytes() and torch.equal(r, r2)
    assert np.array_equal(_np(codes), (up >= 0).astype(np.uint8))
    if dtype == BF16:
        check_dense(out, dense)
    else:
        assert U.same_bits_nan(_np(out), dense)
    assert ops.efsign_step(g[:0], r[:0], False, 1.0, 1.0, want_codes=True)[1].numel() == 0    # n = 0: no launch


# rank means: finite ones with a zero and denormals; inf and one NaN leading, so every world size has them
MEANS = {"finite": [0.75, 0.0, 1e-40, 0.01, 3.0, 0.0, 1.5e-39, 0.2],
         "inf": [np.inf, 0.5, 0.0, 1e-40, 3.0, 0.25, 0.0, 0.2],
         "special": [np.inf, np.nan, 0.0, 1e-40, 3.0, 0.25, 0.0, 0.2]}


@pytest.mark.parametrize("which", sorted(MEANS))
@pytest.mark.parametrize("out_dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("n", [5, 4099, 4100, 262149, 1048580])
@pytest.mark.parametrize("world", [1, 2, 3, 8])
def test_decode_aggregate(world, n, out_dtype, which):
    from grace_amd import ops
    rng = np.random.default_rng(31 * world + n % 1009)
    codes = (rng.random(world * n) < 0.5).astype(np.uint8)
    means = np.array(MEANS[which][:world], dtype=np.float32)
    lr = 0.3
    got = ops.efsign_decode_aggregate(torch.from_numpy(means).to(DEV), torch.from_numpy(codes).to(DEV), world, n, lr,
                                      out_dtype=out_dtype)
    assert got.dtype == out_dtype and got.shape == (n,)
    exp = U.ef_decode_aggregate(means, codes, world, n, lr)
    if out_dtype == BF16:
        check_dense(got, exp)
    else:
        assert U.same_bits_nan(_np(got), exp)
