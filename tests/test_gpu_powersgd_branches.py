"""The unfused PowerSGD kernels (grace_amd/csrc/powersgd.hip: grace_powersgd_p, _p_draw, _qt, _outer,
grace_orthogonalize, grace_normal_fill) on every branch their launchers can take -- the path of
every world size above 1, every rank other than 4 and every matrix the one-pass compress refuses.

Each contraction case names the launch choice it is there for and asserts it against a restatement
of the launcher (tests/powersgd_util.py), runs on a standard normal matrix and on the same matrix
with its rows scaled over twelve decades, and is held to the componentwise bound
2 k u |A| |B| (dot_bound) as well as to the project's bar 1e-5 sqrt(k).  The
outer product is held bit for bit to its f32 chain (tests/device_rng.py outer_f32), and ops.normal to
a float64 restatement of its stream (normal_stream)."""
import numpy as np
import pytest
import torch

from grace_amd import _lib, ops
from tests.device_rng import NORMAL_SEEDS, NORMAL_ZMAX, normal_moment_bounds, normal_stream, outer_f32
from tests.golden_util import same_bits
from tests.powersgd_util import dot_bound, misaligned, orth_rows, p_launch, project_close, qt_launch, workspace_bytes

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _np(t):
    return t.detach().cpu().numpy()


def _exact_qr(a):
    """f64 Householder QR of the (f32) input, columns signed like Gram-Schmidt (R_cc > 0)."""
    q, r = np.linalg.qr(np.asarray(a, dtype=np.float64))
    return q * np.where(np.diag(r) < 0, -1.0, 1.0)


def _inputs(shape, seed):
    """The case's two matrices: standard normal, and the same with rows scaled by 10^U(-6, 6) (the
    global-scale atol of the project bar hides an error in a small row; the componentwise bound
    does not)."""
    rng = np.random.default_rng(seed)
    M = rng.standard_normal(shape, dtype=np.float32)
    s = (10.0 ** rng.uniform(-6, 6, size=(shape[0], 1))).astype(np.float32)
    return rng, (("normal", M), ("rows scaled", M * s))


def _check_product(got, A, B, k, what):
    """got = A @ B (contraction length k) within the project bar and the componentwise bound."""
    ref = A.astype(np.float64) @ B.astype(np.float64)
    err = np.abs(got.astype(np.float64) - ref)
    bound = dot_bound(A, B, k)
    ratio = float((err / np.maximum(bound, 1e-300)).max())
    print(f"{what}: max err / componentwise bound = {ratio:.3g}")
    assert np.isfinite(got).all(), what
    assert project_close(got, ref, k), (what, float(err.max()))
    assert np.all(err <= bound), (what, ratio)


def _expect(launch, want, what, shape, r):
    for key, v in want.items():
        assert launch[key] == v, (what, key, launch)
    # the one figure of the library's own launch arithmetic that can be read back
    n, m = shape
    assert _lib.query("grace_powersgd_workspace_bytes", n, m, r) == workspace_bytes(n, m, r), what


# ------------------------------------------------------------------------------------------ P = M q
def _p_cases():
    c = []
    for r in range(1, 17):     # generic tiles and their col < r mask, 4 K chunks; r = 4 is the rank-4 kernel
        c.append((f"ranks-r{r}", (100, 1000), r, {}, {"kernel": "r4" if r == 4 else "vec", "ksplit": 4, "empty": 0}))
    c += [                     # row / column tails
        ("tiny-1x1", (1, 1), 1, {}, {"kernel": "scalar", "ksplit": 1}),
        ("tiny-1x3", (1, 3), 1, {}, {"kernel": "scalar", "ksplit": 1}),
        ("tiny-17x257-r1", (17, 257), 1, {}, {"kernel": "scalar", "ksplit": 2}),
        ("tiny-17x257-r4", (17, 257), 4, {}, {"kernel": "scalar", "ksplit": 2}),
        ("tiny-16x256-r1", (16, 256), 1, {}, {"kernel": "vec", "ksplit": 1}),
        ("tiny-16x256-r4", (16, 256), 4, {}, {"kernel": "r4", "ksplit": 1}),
        # VEC = false: m % 4 != 0, or M not 16-B aligned
        ("nonvec-m1001", (100, 1001), 4, {}, {"kernel": "scalar", "ksplit": 4}),
        ("nonvec-misaligned-M", (100, 1000), 4, {"mis_M": True}, {"kernel": "scalar", "ksplit": 4}),
        # vec && !r4 at r = 4: q (powersgd_p) or P (p_draw's out=, a send record) not 16-B aligned
        ("r4-off-misaligned-qP", (100, 1000), 4, {"mis_qP": True}, {"kernel": "vec", "r4": False, "ksplit": 4}),
        # 66 column tiles over 64 chunks of 2: chunks 33..63 have kt0 >= kt1 and contribute zeros
        ("empty-chunks-r3", (16, 16641), 3, {}, {"kernel": "scalar", "ksplit": 64, "per": 2, "empty": 31}),
        ("empty-chunks-r4", (16, 16641), 4, {}, {"kernel": "scalar", "ksplit": 64, "per": 2, "empty": 31}),
        # more row tiles than tickets: no K split
        ("tall-r2", ((1 << 20) + 17, 8), 2, {}, {"kernel": "vec", "over_tickets": True, "ksplit": 1}),
        ("tall-r4", ((1 << 20) + 17, 8), 4, {}, {"kernel": "r4", "over_tickets": True, "ksplit": 1}),
        # n * 16 * 64 >= 2^31: rank 4 drops to the generic kernel
        ("r4-guard", (1 << 21, 4), 4, {}, {"kernel": "vec", "r4": False, "over_tickets": True, "ksplit": 1}),
    ]
    return c


@pytest.mark.parametrize("name,shape,r,opt,want", _p_cases(), ids=[c[0] for c in _p_cases()])
def test_p_branches(name, shape, r, opt, want):
    n, m = shape
    mis_M, mis_qP = opt.get("mis_M", False), opt.get("mis_qP", False)
    _expect(p_launch(n, m, r, m_aligned=not mis_M, qp_aligned=not mis_qP), want, name, shape, r)
    rng, inputs = _inputs(shape, 1000 + n % 997 + 31 * m + r)
    q = rng.standard_normal((m, r), dtype=np.float32)
    seed = 4242 + r
    q0 = _np(ops.normal((m, r), seed, DEV))
    for label, M in inputs:
        Md = _t(M)
        if mis_M:
            Md = misaligned(Md)
        qd = _t(q)
        if mis_qP:
            qd = misaligned(qd)
        _check_product(_np(ops.powersgd_p(Md, qd)), M, q, m, f"{name} p [{label}]")
        out = misaligned(torch.zeros(n, r, device=DEV)) if mis_qP else None
        P = ops.powersgd_p_draw(Md, r, seed, out=out)
        if out is not None:
            assert P.data_ptr() == out.data_ptr()
        _check_product(_np(P), M, q0, m, f"{name} p_draw [{label}]")


# --------------------------------------------------------------------------------------- Q = M^T P
def _qt_cases():
    c = []
    for r in range(1, 17):     # r = 4: psgd_qt4_kernel; the others the MFMA kernel (260 r is a multiple of 4: 16-B partials)
        if r == 4:
            want = {"kernel": "qt4", "nslab": 64, "reduce": "v4", "levels": 2, "last_group": 8}
        else:
            want = {"kernel": "vec", "nslab": 128, "reduce": "v4", "levels": 2, "last_group": 8}
        c.append((f"ranks-r{r}", (4096, 260), r, {}, want))
    two = {"nslab": 10, "levels": 2, "last_group": 2}     # 10 slabs: groups of 8 and 2
    c += [
        ("scalar-two-level", (300, 17), 3, {}, {"kernel": "scalar", "reduce": "scalar", **two}),
        ("scalar-two-level-r5", (300, 17), 5, {}, {"kernel": "scalar", "reduce": "scalar", **two}),
        ("scalar-two-level-r15", (300, 17), 15, {}, {"kernel": "scalar", "reduce": "scalar", **two}),
        ("v4-two-level-partial", (300, 16), 3, {}, {"kernel": "vec", "reduce": "v4", **two}),
        ("generic-doubling", (4200, 64), 2, {},
         {"kernel": "vec", "slabs_before": 132, "nslab": 66, "reduce": "v4", "levels": 2, "last_group": 2}),
        ("qt4-two-level", (1000, 64), 4, {}, {"kernel": "qt4", "nslab": 16, "reduce": "v4", "levels": 2, "last_group": 8}),
        ("qt4-doubling", (8300, 64), 4, {},
         {"kernel": "qt4", "slabs_before": 130, "nslab": 65, "reduce": "v4", "levels": 2, "last_group": 1}),
        ("r4-off-qt4-misaligned-P", (1000, 64), 4, {"mis_P": True}, {"kernel": "vec", "nslab": 32, "reduce": "v4"}),
        ("r4-off-qt4-m66", (1000, 66), 4, {}, {"kernel": "scalar", "nslab": 32, "reduce": "v4"}),
        ("single-slab-vec", (40, 65540), 3, {}, {"kernel": "vec", "whole_n": True, "nslab": 1, "reduce": "single"}),
        ("single-slab-scalar", (40, 65541), 3, {}, {"kernel": "scalar", "whole_n": True, "nslab": 1, "reduce": "single"}),
        ("wide-qt4", (40, 65540), 4, {}, {"kernel": "qt4", "groups": 65, "nslab": 1, "reduce": "single"}),
        ("tiny-1x1", (1, 1), 1, {}, {"kernel": "scalar", "nslab": 1}),
        ("tiny-1x8", (1, 8), 1, {}, {"kernel": "vec", "nslab": 1}),
        ("tiny-31x5", (31, 5), 1, {}, {"kernel": "scalar", "nslab": 1}),            # one slab at the floor of 32 rows
        ("tiny-33x5", (33, 5), 1, {}, {"kernel": "scalar", "nslab": 2, "reduce": "scalar", "levels": 1, "last_group": 2}),
    ]
    return c


@pytest.mark.parametrize("name,shape,r,opt,want", _qt_cases(), ids=[c[0] for c in _qt_cases()])
def test_qt_branches(name, shape, r, opt, want):
    n, m = shape
    mis_P = opt.get("mis_P", False)
    _expect(qt_launch(n, m, r, p_aligned=not mis_P), want, name, shape, r)
    rng, inputs = _inputs(shape, 2000 + n % 997 + 31 * m + r)
    P = rng.standard_normal((n, r), dtype=np.float32)      # seeded, not the P kernel's own output
    for label, M in inputs:
        Pd = _t(P)
        if mis_P:
            Pd = misaligned(Pd)
        _check_product(_np(ops.powersgd_qt(_t(M), Pd)), M.T, P, n, f"{name} qt [{label}]")


# ------------------------------------------------------------------------------------ outer product
def _canon(a):
    """NaNs made one pattern: the host's and the device's default NaN differ in sign / payload, which
    is no property of the kernel; every other value, signed zeros included, keeps its bits."""
    a = np.array(a, dtype=np.float32, copy=True)
    a[np.isnan(a)] = np.float32(np.nan)
    return a


def _bits(a, b):
    return same_bits(_canon(a), _canon(b))


def _special(P, Q):
    """NaN, +-inf and -0.0 planted in copies of P and Q; P's row 0 is all -0.0, so the chain
    0 + p q must give +0 there (a chain started from the first product would give -0)."""
    P, Q = P.copy(), Q.copy()
    P[0, :] = -0.0
    vals = np.array([np.nan, np.inf, -np.inf, -0.0], dtype=np.float32)
    for k, v in enumerate(vals):
        if P.shape[0] > 1:
            P.flat[P.shape[1] + (5 * k + 1) % (P.size - P.shape[1])] = v
        Q.flat[(7 * k + 3) % Q.size] = v
    return P, Q


_OUTER = [(f"r{r}-37x1029", (37, 1029), r, {}) for r in range(1, 17)] + [
    ("r4-5x1024", (5, 1024), 4, {}), ("r4-4x1028", (4, 1028), 4, {}), ("r4-1x4", (1, 4), 4, {}),
    ("r4-17x1023", (17, 1023), 4, {}),
    ("r3-37x1028-vec", (37, 1028), 3, {}),                       # generic kernel with 16-B stores
    ("r4-misaligned-P", (17, 1028), 4, {"mis_P": True}),         # generic vector kernel == outer4, bit for bit
    ("r4-misaligned-M", (17, 1028), 4, {"mis_M": True}),         # scalar stores
    ("r3-misaligned-M", (17, 1028), 3, {"mis_M": True}),
    ("r4-misaligned-out", (17, 1028), 4, {"mis_out": True}),
]


@pytest.mark.parametrize("name,shape,r,opt", _OUTER, ids=[c[0] for c in _OUTER])
def test_outer_bit_exact(name, shape, r, opt):
    n, m = shape
    rng = np.random.default_rng(3000 + n + 31 * m + r)
    M = rng.standard_normal(shape, dtype=np.float32)
    P0 = rng.standard_normal((n, r), dtype=np.float32)
    Q0 = rng.standard_normal((m, r), dtype=np.float32)
    Md = misaligned(_t(M)) if opt.get("mis_M") else _t(M)
    for label, (P, Q) in (("normal", (P0, Q0)), ("special", _special(P0, Q0))):
        exp = outer_f32(P, Q)
        with np.errstate(all="ignore"):
            exp_res = M - exp
        assert exp_res.dtype == np.float32
        Pd, Qd = _t(P), _t(Q)
        if label == "special":
            assert not np.signbit(exp[0][~np.isnan(exp[0])]).any()      # the -0.0 row gives +0
        for want_out, want_res in ((True, False), (False, True), (True, True)):
            what = (name, label, want_out, want_res)
            if opt.get("mis_out"):
                ob = misaligned(torch.full((n, m), 7.0, device=DEV)) if want_out else None
                rb = misaligned(torch.full((n, m), 7.0, device=DEV)) if want_res else None
                out, res = ops.powersgd_outer(Pd, Qd, Md if want_res else None, want_out=False, out=ob, residual=rb)
                assert (out is None) == (not want_out) and (res is None) == (not want_res)
                assert out is None or out.data_ptr() == ob.data_ptr()
                assert res is None or res.data_ptr() == rb.data_ptr()
            else:
                out, res = ops.powersgd_outer(Pd, Qd, Md if want_res else None, want_out=want_out,
                                              want_residual=want_res)
            assert (out is not None) == want_out and (res is not None) == want_res, what
            if want_out:
                assert _bits(_np(out), exp), what
            if want_res:
                assert _bits(_np(res), exp_res), what
            if opt.get("mis_P"):      # the generic vector kernel against the aligned rank-4 kernel
                out2, res2 = ops.powersgd_outer(misaligned(Pd), Qd, Md if want_res else None, want_out=want_out,
                                                want_residual=want_res)
                assert out is None or same_bits(_np(out2), _np(out)), what
                assert res is None or same_bits(_np(res2), _np(res)), what


def test_outer_refuses_rank_above_16():
    """r = 17: the kernel's rank loop stops at 16 columns, so the library refuses the call and
    writes nothing (it used to return the product of the first 16 columns)."""
    rng = np.random.default_rng(17)
    P, Q = _t(rng.standard_normal((5, 17), dtype=np.float32)), _t(rng.standard_normal((8, 17), dtype=np.float32))
    M = _t(rng.standard_normal((5, 8), dtype=np.float32))
    out, res = torch.full((5, 8), 7.0, device=DEV), torch.full((5, 8), 7.0, device=DEV)
    with pytest.raises(_lib.GraceNativeError, match="grace_powersgd_outer"):
        ops.powersgd_outer(P, Q, M, out=out, residual=res)
    torch.cuda.synchronize()
    assert (_np(out) == 7.0).all() and (_np(res) == 7.0).all()
    out16, _ = ops.powersgd_outer(P[:, :16], Q[:, :16])                 # 16 is still taken
    assert _bits(_np(out16), outer_f32(_np(P)[:, :16], _np(Q)[:, :16]))


def test_ops_take_strided_operands_and_refuse_other_dtypes():
    """A transposed or strided view used to be read through data_ptr() as if dense (garbage, no
    error): the operands are now made dense first, like q and P always were."""
    rng = np.random.default_rng(23)
    W = rng.standard_normal((300, 200), dtype=np.float32)
    q = rng.standard_normal((300, 3), dtype=np.float32)
    P = rng.standard_normal((300, 3), dtype=np.float32)
    Wd = _t(W)
    assert not Wd.t().is_contiguous()
    _check_product(_np(ops.powersgd_p(Wd.t(), _t(q))), W.T, q, 300, "p of a transposed view")
    _check_product(_np(ops.powersgd_p_draw(Wd.t(), 3, 5)), W.T, _np(ops.normal((300, 3), 5, DEV)), 300, "p_draw of a view")
    Q = rng.standard_normal((200, 3), dtype=np.float32)
    _check_product(_np(ops.powersgd_qt(Wd.t(), _t(Q))), W, Q, 200, "qt of a transposed view")
    P8, Q8 = rng.standard_normal((37, 8), dtype=np.float32), rng.standard_normal((1029, 8), dtype=np.float32)
    M = rng.standard_normal((1029, 37), dtype=np.float32)
    out, res = ops.powersgd_outer(_t(P8)[:, ::2], _t(Q8)[:, ::2], _t(M).t(), want_out=True, want_residual=True)
    exp = outer_f32(P8[:, ::2], Q8[:, ::2])
    assert _bits(_np(out), exp) and _bits(_np(res), M.T - exp)
    assert not ops.powersgd_w1_ok(_t(rng.standard_normal((256, 256), dtype=np.float32)).t(), 4)
    M64 = torch.zeros(8, 8, dtype=torch.float64, device=DEV)
    f = torch.zeros(8, 2, device=DEV)
    for call in (lambda: ops.powersgd_p(M64, f), lambda: ops.powersgd_p_draw(M64, 2, 1),
                 lambda: ops.powersgd_qt(M64, f), lambda: ops.powersgd_w1_compress(M64),
                 lambda: ops.powersgd_outer(f, f, M64, want_residual=True),
                 lambda: ops.powersgd_outer(f.double(), f), lambda: ops.powersgd_p(M64.float(), f.double())):
        with pytest.raises(TypeError):
            call()
    with pytest.raises(ops.GraceDeviceError):
        ops.powersgd_p(torch.zeros(8, 8), f)


# ------------------------------------------------------------------------------------ orthogonalise
def _orth_cases():
    c = [(700, r, False) for r in range(1, 17)]
    # the last register-resident height of each class and the first streamed one
    c += [(n, r, False) for r in (3, 4) for n in (4096, 4097)]
    c += [(n, r, False) for r in (5, 8) for n in (2048, 2049)]
    c += [(n, r, False) for r in (9, 16) for n in (1024, 1025)]
    c += [(r, r, False) for r in (1, 4, 16)]
    c += [(700, 4, True)]          # A not 16-B aligned: the generic <4> kernel, not orth4
    return c


@pytest.mark.parametrize("n,r,mis", _orth_cases())
def test_orthogonalize_branches(n, r, mis):
    """Against the exact f64 QR factor (1e-5) and orthonormal (1e-5); the fused draw equals draw then
    orthogonalise (1e-5)."""
    if not mis and n > r:
        assert (n <= orth_rows(r)) == (n in (700, 1024, 2048, 4096))
    rng = np.random.default_rng(4000 + 17 * n + r)
    a = rng.standard_normal((n, r), dtype=np.float32)
    ad = misaligned(_t(a)) if mis else _t(a)
    out = _np(ops.orthogonalize_(ad))
    assert np.isfinite(out).all()
    assert np.abs(out.T.astype(np.float64) @ out - np.eye(r)).max() < 1e-5
    assert np.abs(out - _exact_qr(a)).max() < 1e-5
    if not mis:
        fused = _np(ops.normal_orthogonal((n, r), 77, DEV))
        ref = _np(ops.orthogonalize_(ops.normal((n, r), 77, DEV)))
        assert np.abs(fused - ref).max() < 1e-5


# ------------------------------------------------------------------------------- workspace contract
def test_workspace_left_zeroed_and_results_reproducible():
    """"Left zeroed by every call" (include/grace_hip.h): after P and after Qt, at shapes that take
    the rank-4 kernels, the scalar and the 16-B two-level reductions, empty K chunks and doubled
    slabs, every ticket is zero again; each call repeated gives identical bits (the partials are
    summed in a fixed order by the last workgroup to arrive), and the first shape run again after
    the others gives the first run's bits."""
    shapes = [((4096, 4096), 4), ((300, 17), 3), ((16, 16641), 3), ((4200, 64), 2), ((4096, 4096), 4)]
    rng = np.random.default_rng(51)
    data = {}
    results = []
    for shape, r in shapes:
        if shape not in data:
            data[shape] = (_t(rng.standard_normal(shape, dtype=np.float32)),
                           _t(rng.standard_normal((shape[1], r), dtype=np.float32)))
        Md, qd = data[shape]
        dev = Md.device

        def tickets_zero():
            ws = ops.workspace("powersgd", 256, dev)
            assert ws.numel() >= 65536 * 4
            return not _np(ws[:65536 * 4]).any()

        Ps = []
        for _ in range(3):
            Ps.append(_np(ops.powersgd_p(Md, qd)))
            assert tickets_zero(), (shape, "P")
        Pd = _t(Ps[0])
        Qs = []
        for _ in range(3):
            Qs.append(_np(ops.powersgd_qt(Md, Pd)))
            assert tickets_zero(), (shape, "Qt")
        assert all(same_bits(Ps[0], x) for x in Ps[1:]) and all(same_bits(Qs[0], x) for x in Qs[1:]), shape
        results.append((Ps[0], Qs[0]))
    assert same_bits(results[0][0], results[-1][0]) and same_bits(results[0][1], results[-1][1])


# ------------------------------------------------------------------------------------ normal stream
# max |z - z64| / max(1, rad) of ops.normal against the float64 restatement, measured on an MI355X at
# n = 2^22 + 1 (both seeds); the test asserts 4x this.  See test_normal_stream_vs_float64.
NORMAL_ERR_MEASURED = 2.56e-7


def _normal_err(z, seed):
    z64, rad = normal_stream(seed, z.size, with_rad=True)
    return float((np.abs(z.astype(np.float64).reshape(-1) - z64) / np.maximum(1.0, rad)).max())


@pytest.mark.parametrize("seed", NORMAL_SEEDS)
@pytest.mark.parametrize("shape", [(1,), (2,), (7,), ((1 << 22) + 1,), (1000, 3)])
def test_normal_stream_vs_float64(shape, seed):
    """ops.normal against normal_stream: the same hash and uniforms, Box-Muller in float64 where the
    kernel uses v_log / v_sqrt / v_sin / v_cos.  Their error is not documented, so the bound is four
    times the measured maximum of |z - z64| / max(1, rad) (NORMAL_ERR_MEASURED above): 2.56e-7 at seed
    4242 and 2.37e-7 at seed 7 over 2^22 + 1 draws on an MI355X, the f32 rounding of z included (the
    source's "a few ulp" holds).  A swap of sin and cos, a wrong log2 scale or a wrong u1 range is an
    error of order 1."""
    z = _np(ops.normal(shape, seed, DEV))
    assert z.shape == tuple(shape) and z.dtype == np.float32
    assert np.isfinite(z).all() and np.abs(z).max() <= NORMAL_ZMAX * (1 + 1e-6)
    err = _normal_err(z, seed)
    print(f"normal {shape} seed {seed}: max |z - z64| / max(1, rad) = {err:.3g}")
    assert err <= 4 * NORMAL_ERR_MEASURED
    if z.size > 1 << 22:
        assert max(normal_moment_bounds(z.reshape(-1)[:1 << 22])) < 1, normal_moment_bounds(z.reshape(-1)[:1 << 22])


# ------------------------------------------------------------------------------ compressor fallbacks
def test_w1_ok_query():
    q = lambda n, m, r: bool(_lib.query("grace_powersgd_w1_ok", n, m, r))      # noqa: E731
    torch.zeros(1, device=DEV)                                                    # the query asks the device for its CUs
    assert q(1 << 20, 8, 4) and q(64, 16384, 4)
    assert not q((1 << 20) + 1, 8, 4) and not q(64, 16388, 4) and not q(64, 10, 4) and not q(64, 16384, 3)


@pytest.mark.parametrize("shape,mis", [((256, 301), False), ((64, 16388), False), ((256, 300), True)])
def test_compressor_falls_back_to_the_unfused_sequence(shape, mis):
    """Matrices the one-pass compress refuses (m % 4 != 0, m > 16384, not 16-B aligned) at world size
    1, rank 4: p_draw -> orthogonalize -> qt, equal to the f64 restatement of the reference algorithm
    on the device draw at the bars of tests/test_gpu_powersgd_w1.py."""
    from grace_amd.dist.compressor.powersgd import PowerSGDCompressor
    n, m = shape
    M = np.random.default_rng(n + m).standard_normal(shape, dtype=np.float32)
    Md = misaligned(_t(M)) if mis else _t(M)
    assert not ops.powersgd_w1_ok(Md, 4)
    called = []
    orig = ops.powersgd_qt
    ops.powersgd_qt = lambda *a, **k: called.append(1) or orig(*a, **k)
    try:
        _, (p, q, _) = PowerSGDCompressor(rank=4).compress(Md, "w")
    finally:
        ops.powersgd_qt = orig
    assert called
    q0 = _np(ops.normal((m, 4), ops.step_seed("powersgd-q", "w", 1), DEV))
    Pe = _exact_qr(M.astype(np.float64) @ q0.astype(np.float64))
    Qe = M.T.astype(np.float64) @ Pe
    assert project_close(_np(p), Pe, m, scale=1.0), np.abs(_np(p) - Pe).max()
    assert project_close(_np(q), Qe, n), np.abs(_np(q) - Qe).max() / np.abs(Qe).max()
