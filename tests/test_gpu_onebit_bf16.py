"""One-bit's kernels of grace_amd/csrc/cast.hip: the bf16 encode, the fused world-1 step and the W-rank
decode for float32 and bfloat16, by the reduction spec in the header of
tests/test_gpu_elementwise.py.

mask0 is exact.  The device sums each class in f64 over a fixed partition; no term cancels within a
class, so its relative error is below n * 2^-53 and the means are within 2 ulp of OneBitFin's f32
formula on the exact sums (math.fsum): 1 ulp for the rounded sum, one more for the quotient.  Two calls
give the same bits.  Everything after the means is exact given the means the device used: the dense
result is 0 + dec(mask0, mean0, mean1) -- two products, then the add, with and without
compat_uint8_not -- and the W-rank decode the rank-ordered f32 sum, divided unless the divisor is 1,
rounded once for a bf16 result.

Sizes as tests/test_gpu_cast_bf16.py.  Each kernel has a size just past one trip of its own grid: the
two passes over x (onebit_sums_e, onebit_apply_e) run at most 1024 workgroups x 256 lanes x 8 bf16 or
4 f32, so WRAP = 2^21 + 5 is past the bf16 wrap and 1,048,579 past the f32 one; the W-rank decode
(onebit_decode_e) runs at most 4096 workgroups, which wrap at 2^23 bf16 or 2^22 f32 elements, so its
test adds DECODE_WRAP = 2^23 + 5, past both."""
import functools

import numpy as np
import pytest
import torch

from grace_amd import _lib, ops
from oracle import grace_oracle as O
from tests import cast_bf16_util as U
from tests.test_gpu_cast_bf16 import BF16, DEV, F32, U8, Slot, cases, torch_round

pytestmark = pytest.mark.gpu
WRAP = (1 << 21) + 5
DECODE_WRAP = (1 << 23) + 5
SIZES = (1, 3, 5, 7, 8, 9, 15, 17, 4099, 65537, 262149, 1048579, WRAP)
NP32 = np.float32


@functools.lru_cache(maxsize=None)
def values(n, kind="mixed"):
    """bf16-representable f32[n], read-only."""
    rng = np.random.default_rng(300 + n % 1000)
    x = U.representable(rng.standard_normal(n).astype(NP32) * np.exp2(rng.integers(-8, 8, n)).astype(NP32))
    if kind == "mixed" and n >= 8:
        x[[0, n // 2, n - 1]] = [0.0, -0.0, 2.0 ** -133]          # ±0 and a bf16 denormal: all "not x < 0"
        x[n // 3] = -(2.0 ** -133)
    elif kind == "mixed":
        x = np.array([-1.5, 0.0, 2.0, -0.0, -3.0, 2.0 ** -133, 0.5], dtype=NP32)[(np.arange(n) + n) % 7]
    elif kind == "no_negative":
        x = np.abs(x)
    elif kind == "all_negative":
        x = -np.maximum(np.abs(x), NP32(2.0 ** -100))
    elif kind == "zeros":
        x = np.where(np.arange(n) % 2 == 0, NP32(0.0), NP32(-0.0)).astype(NP32)
    elif kind == "nan":
        x[n // 2] = np.nan
    elif kind == "inf":
        x[n // 2] = np.inf
    elif kind == "neg_inf":
        x[n // 2] = -np.inf
    x = np.ascontiguousarray(x, dtype=NP32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def exact_means(n, kind="mixed"):
    return U.onebit_fin(*U.onebit_exact_sums(values(n, kind)), n)


def check_means(got, n, kind):
    want = exact_means(n, kind)
    for g, w, which in zip(got, want, ("mean0", "mean1")):
        assert U.ulps_apart(g, w) <= 2, (which, n, kind, float(g), float(w))


def in_slot(x, dtype, off):
    return Slot(x.size, dtype, off, U.narrow(x) if dtype == BF16 else x.view(np.uint32))


def dense_want(x, m, quirk, dtype):
    d = O.python_sum([U.onebit_dec(U.onebit_mask(x), m[0], m[1], quirk)])
    return U.narrow(d) if dtype == BF16 else d


def same_dense(slot, want):
    """Bit for bit (NaN-ness only at a NaN); a message or None."""
    got = slot.bits()
    if slot.dtype == BF16:
        return U.same_bf16(got, want)
    gn, wn = np.isnan(got.view(NP32)), np.isnan(want)
    bad = np.flatnonzero((gn != wn) | ((got != want.view(np.uint32)) & ~wn))
    return None if bad.size == 0 else f"{bad.size} differ, first at {int(bad[0])}"


def ws_for(n):
    nbytes = _lib.query("grace_reduce_workspace_bytes", n)
    return ops.workspace("reduce", nbytes, torch.device(DEV))


# ----------------------------------------------------------------------------- encode
@pytest.mark.parametrize("n,off", cases(SIZES))
def test_encode_bf16(n, off):
    x = values(n)
    xs = in_slot(x, BF16, off)
    runs = []
    for _ in range(2):
        m, means = Slot(n, U8, off), Slot(2, F32, 0)
        _lib.call("grace_onebit_encode_bf16", xs.t.data_ptr(), n, m.t.data_ptr(), means.t.data_ptr(),
                  ws_for(n).data_ptr(), ops._stream())
        assert np.array_equal(m.bits(), U.onebit_mask(x)) and m.guards_intact() and means.guards_intact()
        runs.append(means.bits().copy())
    assert np.array_equal(runs[0], runs[1])                 # the same bits on every call
    check_means(runs[0].view(NP32), n, "mixed")
    assert xs.guards_intact() and np.array_equal(xs.bits(), U.narrow(x))
    if off == 0:
        mask0, means = ops.onebit_encode_grad(xs.t)
        assert np.array_equal(mask0.cpu().numpy(), U.onebit_mask(x))
        assert np.array_equal(means.cpu().numpy().view(np.uint32), runs[0])


# ----------------------------------------------------------------------------- the fused step
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("n,off", cases(SIZES))
def test_step_w1(n, off, dtype):
    x = values(n)
    xs = in_slot(x, dtype, off)
    name = ops._entry("grace_onebit_step_w1", dtype)
    seen = []
    for quirk in (0, 1, 0):
        o, means = Slot(n, dtype, off), Slot(2, F32, 0)
        _lib.call(name, xs.t.data_ptr(), n, quirk, means.t.data_ptr(), o.t.data_ptr(), ws_for(n).data_ptr(),
                  ops._stream())
        m = means.bits().view(NP32)
        seen.append(means.bits().copy())
        msg = same_dense(o, dense_want(x, m, bool(quirk), dtype))
        assert msg is None and o.guards_intact() and means.guards_intact(), (quirk, msg)
    assert np.array_equal(seen[0], seen[1]) and np.array_equal(seen[0], seen[2])
    check_means(seen[0].view(NP32), n, "mixed")
    assert xs.guards_intact()
    if off == 0:
        means, out = ops.onebit_step_w1(xs.t.view(1, n), quirk=True)
        assert out.dtype == dtype and out.shape == (1, n) and np.array_equal(means.cpu().numpy().view(np.uint32), seen[0])
        if dtype == BF16:   # the encode's means are the step's: one partition, one order
            assert np.array_equal(ops.onebit_encode_grad(xs.t)[1].cpu().numpy().view(np.uint32), seen[0])


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("kind", ["no_negative", "all_negative", "zeros", "nan", "inf", "neg_inf"])
@pytest.mark.parametrize("n", [1, 9, 4099])
def test_step_w1_edge_classes(n, kind, dtype):
    """An empty class on each side (its mean is its sum, 0), all ±0, a NaN ("not x < 0": mean1 is NaN
    and so is every element, 0 * NaN), an inf on either side (0 * inf is NaN for the other class)."""
    x = values(n, kind)
    t = torch.from_numpy(x.copy()).to(DEV).to(dtype)
    for quirk in (False, True):
        means, out = ops.onebit_step_w1(t, quirk=quirk)
        m = means.cpu().numpy()
        check_means(m, n, kind)
        got = out.float().cpu().numpy()
        want = O.python_sum([U.onebit_dec(U.onebit_mask(x), m[0], m[1], quirk)])
        want = U.widen(U.narrow(want)) if dtype == BF16 else want
        assert np.array_equal(np.isnan(got), np.isnan(want))
        ok = ~np.isnan(want)
        assert np.array_equal(got[ok].view(np.uint32), want[ok].view(np.uint32)), (kind, quirk)
        if not quirk:
            plain = got
    got = plain         # what follows is about the plain decode (under the quirk 254 * inf is inf, not NaN)
    if kind == "no_negative":
        assert m[0] == 0 and not U.onebit_mask(x).any()
    if kind == "all_negative":
        assert m[1] == 0 and U.onebit_mask(x).all()
    if kind == "zeros":
        assert m[0] == 0 and m[1] == 0 and (got.view(np.uint32) == 0).all()        # 0 + (-0) is +0
    if kind == "nan":
        assert np.isnan(got).all()
    if kind == "inf":       # mean1 is +inf: the elements of the other class are 1 * mean0 + 0 * inf
        assert np.isnan(got[x < 0]).all() and (got[~(x < 0)] == np.inf).all()


# ----------------------------------------------------------------------------- the W-rank decode
@functools.lru_cache(maxsize=4)
def payload(n, world):
    rng = np.random.default_rng(n % 971 + world)
    mask = (rng.random(world * n) < 0.5).astype(np.uint8)
    m0 = -np.abs(rng.standard_normal(world)).astype(NP32)
    m1 = np.abs(rng.standard_normal(world)).astype(NP32)
    if world == 3:
        m1[1] = np.inf                   # 0 * inf: NaN wherever rank 1's mask is set
    if world == 8:
        m0[5], m1[2] = NP32(1e-40), NP32(-0.0)
    return mask, m0, m1


def decode_want(mask, m0, m1, world, n, quirk, divisor, dtype):
    decs = [U.onebit_dec(mask[w * n:(w + 1) * n], m0[w], m1[w], quirk) for w in range(world)]
    with np.errstate(all="ignore"):
        acc = O.python_sum(decs)
        acc = acc if divisor == 1 else (acc / NP32(divisor)).astype(NP32)
    return U.narrow(acc) if dtype == BF16 else acc


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("n,off", cases(SIZES + (DECODE_WRAP,)))
def test_decode_aggregate(n, off, dtype):
    configs = [(w, avg) for w in (1, 2, 3, 8) for avg in (True, False)] if n <= 65537 else [(1, True), (3, True)]
    name = ops._entry("grace_onebit_decode_aggregate", dtype)
    for world, avg in configs:
        divisor = float(world) if avg else 1.0
        mask, m0, m1 = payload(n, world)
        ms = Slot(world * n, U8, off, mask)
        a, b = Slot(world, F32, 0, m0.view(np.uint32)), Slot(world, F32, 0, m1.view(np.uint32))
        for quirk in ((0, 1) if n <= 65537 else (0,)):
            o = Slot(n, dtype, off)
            _lib.call(name, ms.t.data_ptr(), a.t.data_ptr(), b.t.data_ptr(), world, quirk, divisor, o.t.data_ptr(), n,
                      ops._stream())
            msg = same_dense(o, decode_want(mask, m0, m1, world, n, bool(quirk), divisor, dtype))
            assert msg is None and o.guards_intact(), (world, avg, quirk, msg)
        assert ms.guards_intact() and np.array_equal(ms.bits(), mask)
    if off == 0:
        out = ops.onebit_decode_aggregate(ms.t, a.t, b.t, world, n, quirk=bool(quirk), divisor=divisor, out_dtype=dtype)
        assert out.dtype == dtype and out.shape == (n,)
        if dtype == BF16:      # through torch's cast, which need not keep a NaN's pattern: NaN-ness only there
            assert U.same_bf16(torch_round(out.float()), o.bits()) is None
        else:
            assert np.array_equal(out.cpu().numpy().view(np.uint32), o.bits())


def test_decode_of_the_f32_class_payload_is_the_f32_class_result():
    """The decode launch against the f32 class's own path (decode per rank, rank-ordered sum, divide)
    on payloads the f32 encode wrote."""
    n, world = 4099, 3
    xs = [torch.from_numpy(values(n)[::-1].copy() * NP32(r + 1)).to(DEV) for r in range(world)]
    enc = [ops.onebit_encode(x) for x in xs]
    for quirk in (False, True):
        decs = [ops.onebit_decode(m, means[0:1], means[1:2], quirk=quirk) for m, means in enc]
        ref = ops.div_scalar(ops.sum_rank_order(decs), world)
        mask = torch.cat([m for m, _ in enc])
        m0, m1 = torch.cat([mm[0:1] for _, mm in enc]), torch.cat([mm[1:2] for _, mm in enc])
        out = ops.onebit_decode_aggregate(mask, m0, m1, world, n, quirk=quirk, divisor=world)
        assert torch.equal(out.view(torch.int32), ref.view(torch.int32))
        outb = ops.onebit_decode_aggregate(mask, m0, m1, world, n, quirk=quirk, divisor=world, out_dtype=BF16)
        assert np.array_equal(torch_round(outb.float()), torch_round(ref))
