"""The small kernels every codec runs on (grace_amd/csrc/elementwise.hip), past the golden sizes.

Part 1, the streaming driver op by op: ``stream_kernel<true>`` (16 B per lane) and
``stream_kernel<false>`` (the scalar loop an operand that is not 16-B aligned -- 4-B for u8 codes --
selects) behind axpby, sub, div_scalar, accumulate, the sign family and one-bit.  One shared case
generator: n in SIZES (BIG = 2 * 2^21 + 4 * 1000 + 3 is two full grid-stride trips, a partial third
and a 3-element tail on the vector path, nine trips on the scalar path) times the layouts "every
operand aligned", "each operand in turn a buf[1:] view" and "every operand offset" (BIG: the first
and the last only).  Values are standard normal with +-0, +-NaN, +-inf and +-1e-45 planted at both
ends and inside (n < 8: a run of the specials).  Expected values are numpy / torch-CPU float32 with
one rounding per operation, through the oracle where it has the function; results are compared bit
for bit (NaN positions by NaN-ness), inputs must come back unchanged, and the elements either side of
every operand must still hold their sentinel.

Part 2, the two-stage f64 reductions (``reduce_partials`` / ``reduce_finish``, ``sumsq_kernel``)
against the exact sum (math.fsum over the f64-widened inputs) rounded to f32 and finished with the
kernel's own f32 formula.  The device accumulates in f64 in another order; no term of |x|, x[x < 0],
x[!(x < 0)] or x^2 cancels, so its relative error is below n * 2^-53 ~ 2^-33 and its f32 rounding can
differ from the exact sum's only when that sum lies within 2^-33 of a rounding boundary: the bar is
1 ulp for a sum and 2 ulp for a mean (one more rounding in the quotient).  The project's bars against
torch's CPU f32 cascades (2 ulp EF mean, 4 ulp one-bit means and sumsq) stay as a second assertion
for n <= 65,537, where that cascade is itself accurate.
"""
import functools
import math

import numpy as np
import pytest
import torch

from grace_amd import ops
from oracle import grace_oracle as O
from tests.golden_util import same_bits

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = np.float32
T32, TU8 = torch.float32, torch.uint8
BIG = 2 * (1 << 21) + 4 * 1000 + 3
SIZES = (1, 2, 3, 4, 5, 1023, 1024, 4099, BIG)
SPECIALS = np.array([0.0, -0.0, np.nan, -np.nan, np.inf, -np.inf, 1e-45, -1e-45], dtype=F32)
SUBNORMAL_QUOTIENTS = (3e-38, -3e-38, 1.2e-38, 8e-38)     # / 3, 7, 8, 16 are subnormal, not zero
SENT_F32, SENT_U8 = -7777.25, 0xA5
GUARD = 4      # sentinel elements either side of an operand; 4 f32 = 16 B keeps the view aligned


def _np(t):
    return t.detach().cpu().numpy()


# ----------------------------------------------------------------------------- the shared cases
@functools.lru_cache(maxsize=None)
def values(n, seed=0, extra=()):
    """f32[n], read-only: standard normal with SPECIALS (+ extra) planted at both ends and inside
    (tests/test_gpu_sign.py::_planted); n < 8: a run of the pool starting at its element 3 * seed."""
    pool = np.concatenate([SPECIALS, np.asarray(extra, dtype=F32)])
    if n < 8:
        x = pool[(np.arange(n) + 3 * seed) % pool.size].copy()
    else:
        x = np.random.default_rng(7000 + 31 * seed + n % 1000).standard_normal(n).astype(F32)
        for base in (0, n // 3, n // 2 + 1, n - pool.size):
            x[base:base + pool.size] = pool
    x.setflags(write=False)
    return x


class Slot:
    """n elements of a device buffer with GUARD sentinel elements either side.  off=False: the view
    starts 16-B aligned; off=True: one element later, a ``buf[1:]`` view (+4 B for f32, +1 B for
    u8), which must select the scalar driver."""

    def __init__(self, n, dtype, off, data=None):
        self.sent = SENT_U8 if dtype == TU8 else SENT_F32
        self.buf = torch.full((n + 2 * GUARD + 1,), self.sent, dtype=dtype, device=DEV)
        self.lo, self.n = GUARD + (1 if off else 0), n
        self.t = self.buf[self.lo:self.lo + n]
        assert self.buf.data_ptr() % 16 == 0 and self.t.is_contiguous()
        step = self.t.element_size()
        assert self.t.data_ptr() % 16 == (GUARD * step + (step if off else 0)) % 16
        if data is not None:
            self.t.copy_(torch.from_numpy(np.array(data)))

    def np(self):
        return _np(self.t)

    def guards_intact(self):
        b = _np(self.buf)
        return bool((b[:self.lo] == self.sent).all() and (b[self.lo + self.n:] == self.sent).all())


def cases(*operands):
    """(n, layout) for an op with these operands: "aligned", "off:<operand>" for each in turn,
    "off:all"; BIG runs the first and the last only."""
    out = []
    for n in SIZES:
        lays = ["aligned", "off:all"]
        if n != BIG and len(operands) > 1:
            lays[1:1] = [f"off:{o}" for o in operands]
        out += [pytest.param(n, lay, id=f"n{n}-{lay}") for lay in lays]
    return out


def is_off(layout, operand):
    return layout in ("off:all", f"off:{operand}")


def check(got, exp, what=""):
    """Bit for bit; at NaN positions NaN-ness only (tests/test_gpu_topk_bf16.py::check_dense)."""
    got = _np(got) if isinstance(got, torch.Tensor) else np.asarray(got)
    exp = np.ascontiguousarray(exp)
    assert got.shape == exp.shape and got.dtype == exp.dtype, (what, got.shape, exp.shape, got.dtype, exp.dtype)
    if exp.dtype != F32:
        bad = np.flatnonzero(got != exp)
        assert bad.size == 0, (what, "first mismatch at", int(bad[0]), got[bad[0]], exp[bad[0]])
        return
    gn, en = np.isnan(got), np.isnan(exp)
    bad = np.flatnonzero(gn != en)
    assert bad.size == 0, (what, "NaN positions differ, first at", int(bad[0]), got[bad[0]], exp[bad[0]])
    bad = np.flatnonzero((got.view(np.uint32) != exp.view(np.uint32)) & ~en)
    assert bad.size == 0, (what, bad.size, "elements differ, first at", int(bad[0]), got[bad[0]], exp[bad[0]])


def untouched(slot, orig, what=""):
    """An input holds its original bits (NaN payloads too) and its guards their sentinel."""
    assert same_bits(slot.np(), orig), (what, "input modified")
    assert slot.guards_intact(), (what, "wrote outside the operand")


def quiet(f, *a, **k):
    """f(*a) without numpy's warnings about the planted NaN / inf arithmetic."""
    with np.errstate(all="ignore"):
        return f(*a, **k)


def signs_of(x):
    """signSGD's whole W=1 pipeline on the oracle: aggregate([decode(encode(x))])."""
    return O.sign_aggregate([O.sign_decode(O.sign_encode(x))])


# ----------------------------------------------------------------------------- memory arithmetic
@pytest.mark.parametrize("n,layout", cases("r", "g", "out"))
def test_axpby(n, layout):
    """t = f32(f32(beta r) + f32(gamma g)), no FMA (memory/residual.py:10-14), into a new tensor, into
    g (PowerSGDMemory's call) and into r."""
    r0, g0 = values(n, 0), values(n, 1)
    for beta, gamma in ((1, 1), (0.9, 0.5), (1, 0.1)):
        exp = O.residual_compensate(g0, r0, beta, gamma)
        for mode in ("fresh", "alias_g", "alias_r"):
            if mode != "fresh" and layout == "off:out":
                continue        # the output is an input there: the other layouts cover it
            r, g = Slot(n, T32, is_off(layout, "r"), r0), Slot(n, T32, is_off(layout, "g"), g0)
            o = {"fresh": Slot(n, T32, is_off(layout, "out")), "alias_g": g, "alias_r": r}[mode]
            what = (beta, gamma, mode)
            assert ops.axpby(r.t, g.t, beta, gamma, out=o.t) is o.t
            check(o.t, exp, what)
            assert o.guards_intact(), what
            if o is not r:
                untouched(r, r0, what)
            if o is not g:
                untouched(g, g0, what)


@pytest.mark.parametrize("n,layout", cases("t", "d", "out"))
def test_sub(n, layout):
    """r' = t - d (memory/residual.py:16-20), into a new tensor and into t."""
    t0, d0 = values(n, 0), values(n, 1)
    exp = quiet(O.residual_update, t0, d0)
    for mode in ("fresh", "alias_t"):
        if mode != "fresh" and layout == "off:out":
            continue
        t, d = Slot(n, T32, is_off(layout, "t"), t0), Slot(n, T32, is_off(layout, "d"), d0)
        o = Slot(n, T32, is_off(layout, "out")) if mode == "fresh" else t
        assert ops.sub(t.t, d.t, out=o.t) is o.t
        check(o.t, exp, mode)
        assert o.guards_intact(), mode
        untouched(d, d0, mode)
        if o is not t:
            untouched(t, t0, mode)


@pytest.mark.parametrize("n,layout", cases("x", "out"))
def test_div_scalar(n, layout):
    """x / d, correctly rounded as numpy's f32 division: world sizes and EF-signSGD's learning rate;
    a subnormal quotient (3e-38 / 7) is rounded, not flushed."""
    seeds = (0, 3) if n < 8 else (0,)          # n < 8: a second run reaches the subnormal quotients
    for seed in seeds:
        x0 = values(n, seed, SUBNORMAL_QUOTIENTS)
        for d in (1, 2, 3, 7, 8, 16, 0.1):
            exp = quiet(np.divide, x0, F32(d))
            if d in (3, 7, 8, 16) and (n >= 8 or (seed == 3 and n >= 3)):
                tiny = np.abs(exp[np.isfinite(exp)])
                assert ((tiny > 0) & (tiny < F32(1.1754944e-38))).sum() >= 2, "no subnormal quotient in the case"
            x, o = Slot(n, T32, is_off(layout, "x"), x0), Slot(n, T32, is_off(layout, "out"))
            assert ops.div_scalar(x.t, d, out=o.t) is o.t
            check(o.t, exp, (seed, d))
            assert o.guards_intact(), d
            untouched(x, x0, d)


def _sum_cases():
    out = []
    for count in (1, 2, 3, 8):
        for n in SIZES:
            lays = ["aligned", "off:all"]
            if n != BIG and count > 1:
                lays[1:1] = [f"off:{j}" for j in range(count)]
            out += [pytest.param(count, n, lay, id=f"w{count}-n{n}-{lay}") for lay in lays]
    return out


@pytest.mark.parametrize("count,n,layout", _sum_cases())
def test_sum_rank_order(count, n, layout):
    """Python ``sum``: ((0 + t0) + t1) + ... (grace_dl/dist/__init__.py:32-34); the first launch
    ignores the accumulator, the rest accumulate in place; 0 + -0.0 is +0.0."""
    xs0 = [values(n, j) for j in range(count)]
    exp = quiet(O.python_sum, xs0)
    xs = [Slot(n, T32, is_off(layout, str(j)), x) for j, x in enumerate(xs0)]
    out = ops.sum_rank_order([s.t for s in xs])
    check(out, exp)
    if count == 1:
        zeros = xs0[0] == 0
        assert n < 2 or np.signbit(xs0[0][zeros]).any(), "no -0.0 in the case"
        assert not np.signbit(_np(out)[zeros]).any()
    for s, x in zip(xs, xs0):
        untouched(s, x)


# ----------------------------------------------------------------------------- sign family
@pytest.mark.parametrize("n,layout", cases("x", "out"))
def test_sign_encode(n, layout):
    x0 = values(n, 0)
    x, c = Slot(n, T32, is_off(layout, "x"), x0), Slot(n, TU8, is_off(layout, "out"))
    assert ops.sign_encode(x.t, out=c.t) is c.t
    check(c.t, O.sign_encode(x0))
    assert c.guards_intact()
    untouched(x, x0)
    if layout == "aligned":
        check(ops.sign_encode(x.t), O.sign_encode(x0), "allocated output")


@pytest.mark.parametrize("at", [0, 1, 2, 3])
@pytest.mark.parametrize("n", [1, 5, 1023, 1024, 4099])
def test_sign_encode_into_a_record(n, at):
    """``out=`` a view into a larger u8 send record, 0 to 3 bytes past a word boundary: only
    offset 0 may take the 32-bit store path, and nothing outside the view is written."""
    x0 = values(n, 1)
    rec = torch.full((n + 8,), SENT_U8, dtype=TU8, device=DEV)
    assert rec.data_ptr() % 4 == 0
    ops.sign_encode(torch.from_numpy(np.array(x0)).to(DEV), out=rec[at:at + n])
    got = _np(rec)
    check(got[at:at + n], O.sign_encode(x0))
    assert (got[:at] == SENT_U8).all() and (got[at + n:] == SENT_U8).all()


@pytest.mark.parametrize("n,layout", cases("codes"))
def test_sign_decode(n, layout):
    """u8 * 2 - 1 (signsgd.py:21), and scale * that with a 1-element device scale (efsignsgd.py:26-27),
    a NaN and a -0.0 scale included."""
    c0 = O.sign_encode(values(n, 2))
    c = Slot(n, TU8, is_off(layout, "codes"), c0)
    check(ops.sign_decode(c.t), O.sign_decode(c0), "no scale")
    for s in (0.5, -3.25, np.nan, -0.0, np.inf):
        scale = np.array([s], dtype=F32)
        got = ops.sign_decode(c.t, scale=torch.from_numpy(scale).to(DEV))
        check(got, quiet(O.efsign_decode, scale, c0), s)
    untouched(c, c0)


def _majority_cases():
    out = []
    for world in (1, 2, 3, 8):
        for n in SIZES:
            if n == BIG and world == 8:
                continue            # 8 * BIG codes is a 34 MB buffer; worlds 1 to 3 make the same trips
            out += [pytest.param(world, n, lay, id=f"w{world}-n{n}-{lay}") for lay in ("aligned", "off:codes")]
    return out


@pytest.mark.parametrize("world,n,layout", _majority_cases())
def test_sign_majority(world, n, layout):
    """The majority vote over W gathered code rows (signsgd.py:25-30): rows start at w * n, so the
    32-bit path needs n % 4 == 0 as well as an aligned buffer."""
    rows = [O.sign_encode(values(n, w)) for w in range(world)]
    c0 = np.concatenate(rows)
    c = Slot(world * n, TU8, is_off(layout, "codes"), c0)
    exp = O.sign_aggregate([O.sign_decode(r) for r in rows])
    check(ops.sign_majority(c.t, world, n), exp)
    untouched(c, c0)


@pytest.mark.parametrize("n,layout", cases("g", "m"))
def test_signum_encode(n, layout):
    """Three steps on one momentum buffer (signum.py:19-24): m = g, then m = (1 - 0.9) g + 0.9 m,
    updated in place; the codes are (m >= 0).  The first step must not read the buffer."""
    m = Slot(n, T32, is_off(layout, "m"), np.full(n, np.nan, dtype=F32))
    prev = None
    for step in range(3):
        g0 = values(n, step)
        g = Slot(n, T32, is_off(layout, "g"), g0)
        codes = ops.signum_encode(g.t, m.t, step > 0, 0.9)
        prev = quiet(O.signum_momentum, g0, prev, 0.9)
        check(m.t, prev, ("momentum", step))
        check(codes, O.sign_encode(prev), ("codes", step))
        assert m.guards_intact(), step
        untouched(g, g0, step)


@pytest.mark.parametrize("want_codes", [True, False], ids=["codes", "nocodes"])
@pytest.mark.parametrize("n,layout", cases("x"))
def test_sign_step_w1(n, layout, want_codes):
    """The W=1 sign step: without codes an aligned x of n >= 4 takes sign_step_w1_kernel, anything
    else (an offset x, n < 4, codes wanted) the generic driver; all give the oracle's bits."""
    x0 = values(n, 1)
    x = Slot(n, T32, is_off(layout, "x"), x0)
    codes, out = ops.sign_step_w1(x.t, want_codes=want_codes, reuse_out=False)
    check(out, signs_of(x0))
    if want_codes:
        check(codes, O.sign_encode(x0))
    else:
        assert codes is None
    untouched(x, x0)


# ----------------------------------------------------------------------------- one-bit
@pytest.mark.parametrize("n,layout", cases("x"))
def test_onebit_encode_mask(n, layout):
    """mask0 = (x < 0), NaN in neither class's mask (onebit.py:13-14); the means are checked below."""
    x0 = values(n, 0)
    x = Slot(n, T32, is_off(layout, "x"), x0)
    mask0, _ = ops.onebit_encode(x.t)
    check(mask0, quiet(O.onebit_compress, x0)[0])
    untouched(x, x0)


@pytest.mark.parametrize("quirk", [False, True], ids=["fixed", "quirk"])
@pytest.mark.parametrize("n,layout", cases("mask"))
def test_onebit_decode(n, layout, quirk):
    """mask0 * mean0 + ~mask0 * mean1 as two products and an add (onebit.py:26-30), ~ as 1 - b or the
    dist flavour's uint8 255 - b; NaN, +-inf and -0.0 means."""
    m0 = (values(n, 3) < 0).astype(np.uint8)
    m = Slot(n, TU8, is_off(layout, "mask"), m0)
    for mean0, mean1 in ((-0.5, 1.5), (np.nan, 1.0), (-1.0, np.nan), (-np.inf, np.inf), (np.inf, 2.0),
                         (-0.0, 0.0), (-0.0, -0.0), (0.0, -3.0)):
        a, b = (torch.tensor([v], dtype=T32, device=DEV) for v in (mean0, mean1))
        exp = quiet(O.onebit_decode, m0, F32(mean0), F32(mean1), quirk)
        check(ops.onebit_decode(m.t, a, b, quirk=quirk), exp, (mean0, mean1))
    untouched(m, m0)


# ----------------------------------------------------------------------------- reductions
RED_SIZES = (1, 63, 64, 65, 255, 256, 257, 65_537, 262_144, 262_149, 1_048_579)
RED_SEEDS = (0, 1, 2)
TORCH_BAR_MAX_N = 65_537


def _fsum(a):
    return math.fsum(np.asarray(a, dtype=np.float64).tolist())


def exact_sums(x):
    """The four sums the kernels form, exactly: |x|; x where x < 0 and how many; x where not x < 0
    (NaN counted there); x^2 (an f32 squared is exact in f64)."""
    d = x.astype(np.float64)
    with np.errstate(all="ignore"):
        neg = x < 0
        return {"abs": _fsum(np.abs(d)), "sum0": _fsum(d[neg]), "num0": int(neg.sum()), "sum1": _fsum(d[~neg]),
                "sq": _fsum(d * d)}


@functools.lru_cache(maxsize=None)
def red_case(n, seed):
    x = np.random.default_rng(1000 * seed + n).standard_normal(n).astype(F32)
    x.setflags(write=False)
    return x, exact_sums(x)


def fin_abs_mean(ex, n):
    """AbsMeanFin: (float)sum / (float)n."""
    with np.errstate(all="ignore"):
        return F32(F32(ex["abs"]) / F32(n))


def fin_onebit(ex, n):
    """OneBitFin: num > 0 ? sum / num : sum for both classes, num1 = (float)n - num0."""
    with np.errstate(all="ignore"):
        sum0, num0, sum1 = F32(ex["sum0"]), F32(ex["num0"]), F32(ex["sum1"])
        num1 = F32(F32(n) - num0)
        return (F32(sum0 / num0) if num0 > 0 else sum0), (F32(sum1 / num1) if num1 > 0 else sum1)


def ulps_apart(a, b):
    """Distance of two finite f32 in units in the last place (for the printed figures)."""
    def key(v):
        i = int(np.array(v, dtype=F32).view(np.int32))
        return i if i >= 0 else -(i & 0x7FFFFFFF)
    return abs(key(a) - key(b))


def close(got, want, bar, what):
    print(f"{what}: got {float(got)!r} want {float(want)!r} ({ulps_apart(got, want)} ulp, bar {bar})")
    assert ops.isclose_f32_ulps(np.array(got, dtype=F32), np.array(want, dtype=F32), bar), (what, got, want)


def run_reduction(target, xt):
    """The device's f32 results of one reduction target, as numpy scalars."""
    if target == "abs_mean":
        return (_np(ops.abs_mean(xt))[0],)
    if target == "onebit_means":
        m = _np(ops.onebit_encode(xt)[1])
        return m[0], m[1]
    return (_np(ops.sumsq(xt))[0],)


def want_reduction(target, ex, n):
    if target == "abs_mean":
        return (fin_abs_mean(ex, n),)
    if target == "onebit_means":
        return fin_onebit(ex, n)
    return (F32(ex["sq"]),)


def torch_reduction(target, x):
    """The reference's own f32 expressions on the CPU (efsignsgd.py:17, onebit.py:13-23, memory/dgc.py:18)."""
    t = torch.from_numpy(np.array(x))
    if target == "abs_mean":
        return (t.abs().mean().numpy(),)
    if target == "onebit_means":
        return O.onebit_compress(x)[1:]
    return (torch.sum(t * t).numpy(),)


EXACT_BAR = {"abs_mean": 2, "onebit_means": 2, "sumsq": 1}
TORCH_BAR = {"abs_mean": 2, "onebit_means": 4, "sumsq": 4}


@pytest.mark.parametrize("seed", RED_SEEDS)
@pytest.mark.parametrize("n", RED_SIZES)
@pytest.mark.parametrize("target", ["abs_mean", "onebit_means", "sumsq"])
def test_reduction_against_exact_sum(target, n, seed):
    """65,537 elements are 257 partials (reduce_finish's second trip), 262,149 make reduce_partials
    stride, 1,048,579 is four trips and a ragged end; an aligned tensor and a buf[1:] view."""
    x0, ex = red_case(n, seed)
    want = want_reduction(target, ex, n)
    for off in (False, True):
        x = Slot(n, T32, off, x0)
        got = run_reduction(target, x.t)
        for j, (g, w) in enumerate(zip(got, want)):
            close(g, w, EXACT_BAR[target], f"{target}[{j}] n={n} seed={seed} off={off} vs exact")
        if n <= TORCH_BAR_MAX_N:
            for j, (g, w) in enumerate(zip(got, torch_reduction(target, x0))):
                close(g, w, TORCH_BAR[target], f"{target}[{j}] n={n} seed={seed} off={off} vs torch f32")
        untouched(x, x0)


def _all_targets(xt):
    return {t: run_reduction(t, xt) for t in ("abs_mean", "onebit_means", "sumsq")}


@pytest.mark.parametrize("off", [False, True], ids=["aligned", "offset"])
def test_reduction_one_class_empty(off):
    """All-negative and all-non-negative x: the empty class's mean is its sum, +0.0."""
    n = 65_537
    mag = np.abs(red_case(n, 0)[0]) + F32(0.25)
    for x0, empty in ((-mag, 1), (mag, 0)):
        ex = exact_sums(x0)
        means = run_reduction("onebit_means", Slot(n, T32, off, x0).t)
        assert same_bits(np.array(means[empty], dtype=F32), np.array(0.0, dtype=F32)), means
        close(means[1 - empty], fin_onebit(ex, n)[1 - empty], 2, f"mean{1 - empty}, other class empty")
    zeros = np.array([0.0, -0.0] * 50, dtype=F32)        # +-0 are "not x < 0": class 0 stays empty
    means = run_reduction("onebit_means", Slot(zeros.size, T32, off, zeros).t)
    assert same_bits(np.array(means, dtype=F32), np.zeros(2, dtype=F32)), means


@pytest.mark.parametrize("off", [False, True], ids=["aligned", "offset"])
def test_reduction_nan_and_inf(off):
    """One NaN: mean1 (the class of not x < 0) and the abs-mean and the sum of squares are NaN, mean0
    is the bits it has without it.  One +inf / -inf: its class's mean and the abs-mean and the sum of
    squares are that infinity's, the other class's mean is untouched."""
    n = 65_537
    base = np.array(red_case(n, 1)[0])
    k = n // 2
    base[k] = 1.0
    m0_base, m1_base = run_reduction("onebit_means", Slot(n, T32, off, base).t)
    x0 = base.copy()
    x0[k] = np.nan
    got = _all_targets(Slot(n, T32, off, x0).t)
    assert np.isnan(got["abs_mean"][0]) and np.isnan(got["sumsq"][0]) and np.isnan(got["onebit_means"][1]), got
    assert same_bits(np.array(got["onebit_means"][0]), np.array(m0_base)), (got, m0_base)
    x0[k] = np.inf
    got = _all_targets(Slot(n, T32, off, x0).t)
    assert got["abs_mean"][0] == np.inf and got["sumsq"][0] == np.inf and got["onebit_means"][1] == np.inf, got
    assert same_bits(np.array(got["onebit_means"][0]), np.array(m0_base)), (got, m0_base)
    x0[k] = -np.inf
    base[k] = -1.0                                   # the same count in class 0, a finite member
    m1_base = run_reduction("onebit_means", Slot(n, T32, off, base).t)[1]
    got = _all_targets(Slot(n, T32, off, x0).t)
    assert got["abs_mean"][0] == np.inf and got["sumsq"][0] == np.inf and got["onebit_means"][0] == -np.inf, got
    assert same_bits(np.array(got["onebit_means"][1]), np.array(m1_base)), (got, m1_base)


@pytest.mark.parametrize("off", [False, True], ids=["aligned", "offset"])
def test_reduction_constant_one(off):
    """1,048,579 ones: the abs-mean is exactly 1.0 and the sum of squares exactly 1,048,579.0."""
    n = 1_048_579
    got = _all_targets(Slot(n, T32, off, np.ones(n, dtype=F32)).t)
    assert got["abs_mean"][0] == F32(1.0) and got["sumsq"][0] == F32(n), got
    assert same_bits(np.array(got["onebit_means"], dtype=F32), np.array([0.0, 1.0], dtype=F32)), got


def test_reduction_workspace_reuse():
    """A large reduction then a small one on the same shared workspace, then the reverse order: the
    larger call's stale partials must not leak into the smaller, whose results stay the same bits."""
    (big0, _), (small0, ex) = red_case(1_048_579, 0), red_case(5, 0)
    big, small = Slot(big0.size, T32, False, big0), Slot(small0.size, T32, False, small0)
    seen = []
    for order in ((big, small), (small, big), (big, small)):
        for x in order:
            got = _all_targets(x.t)
            if x is small:
                seen.append(np.array(got["abs_mean"] + got["onebit_means"] + got["sumsq"], dtype=F32))
    for j, target in enumerate(("abs_mean", "onebit_means", "onebit_means", "sumsq")):
        want = (want_reduction("abs_mean", ex, 5) + want_reduction("onebit_means", ex, 5)
                + want_reduction("sumsq", ex, 5))[j]
        close(seen[0][j], want, EXACT_BAR[target], f"small after large [{j}]")
    assert same_bits(seen[0], seen[1]) and same_bits(seen[0], seen[2]), seen
