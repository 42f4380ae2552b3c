"""GPU parity of PowerSGD (grace_amd/csrc/powersgd.hip, f32 MFMA) against golden vectors, within
the f32 tolerance rel <= 1e-5 * sqrt(m) stated in SURVEY.md §8a (different summation orders)."""
import numpy as np
import pytest
import torch

from grace_amd import ops
from oracle import grace_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _np(t):
    return t.detach().cpu().numpy()


def _close(a, b, m, scale=None):
    tol = 1e-5 * np.sqrt(m)
    scale = np.abs(b).max() if scale is None else scale
    return np.allclose(a, b, rtol=tol, atol=tol * max(scale, 1e-30))


@pytest.mark.parametrize("shape", [(64, 48), (33, 17), (256, 256), (100, 1000), (4096, 4096)])
@pytest.mark.parametrize("r", [1, 2, 4])
def test_p_and_qt_vs_numpy(shape, r):
    rng = np.random.default_rng(shape[0] + r)
    M = rng.standard_normal(shape).astype(np.float32)
    q = rng.standard_normal((shape[1], r)).astype(np.float32)
    P = _np(ops.powersgd_p(_t(M), _t(q)))
    Pe = (M.astype(np.float64) @ q.astype(np.float64))
    assert _close(P, Pe, shape[1])
    Q = _np(ops.powersgd_qt(_t(M), _t(P)))
    Qe = M.T.astype(np.float64) @ P.astype(np.float64)
    assert _close(Q, Qe, shape[0])
    out, res = ops.powersgd_outer(_t(P), _t(Q), _t(M), want_out=True, want_residual=True)
    Oe = P.astype(np.float64) @ Q.T.astype(np.float64)
    assert _close(_np(out), Oe, r)
    assert np.array_equal(_np(res), M - _np(out))          # one f32 subtraction: bit-exact


def _exact_qr(a):
    """f64 Householder QR of the (f32) input, columns signed like Gram-Schmidt (R_cc > 0)."""
    q, r = np.linalg.qr(np.asarray(a, dtype=np.float64))
    return q * np.where(np.diag(r) < 0, -1.0, 1.0)


def test_orthogonalize_golden(golden):
    """Well-conditioned reference cases: within 1e-4 of the reference's f32 MGS.  Ill-conditioned
    ones (kappa 1e4 / 1e7, two nearly collinear columns, P of a rank-2 gradient): the reference's own
    f32 MGS is only determined to ~kappa * eps32 in the late columns (its distance from the exact
    factor is measured here), so each column must match the reference within 1e-4 OR within 4x the
    reference's own error, whichever is larger; and the result must be finite and orthonormal (the
    one-pass Cholesky-QR gave NaN / lost orthogonality there before the MGS2 fallback)."""
    cases = golden.cases("powersgd", codec="orthogonalize")
    assert {c.name for c in cases} >= {"orth_ill_4096x4_k10000", "orth_ill_4096x4_k1e+07", "orth_collinear_4096x4",
                                       "orth_rank2_4096x4", "orth_ill_500x3_k10000"}
    for c in cases:
        a = _t(c["a"])
        ops.orthogonalize_(a)
        out = _np(a)
        ref = c["out"]
        assert np.isfinite(out).all(), c.name
        r = out.shape[1]
        assert np.abs(out.T.astype(np.float64) @ out - np.eye(r)).max() < 1e-5, c.name
        if "kappa" not in c.meta:
            assert np.allclose(out, ref, rtol=1e-4, atol=1e-5), c.name
            continue
        qx = _exact_qr(c["a"])
        ref_err = np.abs(ref - qx).max(axis=0)
        ours = np.abs(out - ref).max(axis=0)
        assert np.all(ours <= np.maximum(1e-4, 4 * ref_err)), (c.name, ours, ref_err)
        assert np.abs(out - qx).max() < 1e-5, c.name           # and it IS the exact factor


@pytest.mark.parametrize("n,r,kappa", [(9000, 4, 1e7), (4096, 4, 1e6), (3000, 3, 1e9), (600, 8, 1e7)])
def test_orthogonalize_ill_conditioned_vs_exact_qr(n, r, kappa):
    """Both kernels (rank-4 register path, generic chunked path) on inputs with condition number
    up to 1e9: finite, orthonormal, equal to the exact QR factor of the f32 input."""
    rng = np.random.default_rng(int(np.log10(kappa)) + n)
    u, _ = np.linalg.qr(rng.standard_normal((n, r)))
    v, _ = np.linalg.qr(rng.standard_normal((r, r)))
    a = ((u * np.logspace(0, -np.log10(kappa), r)) @ v.T).astype(np.float32)
    out = _np(ops.orthogonalize_(_t(a)))
    assert np.isfinite(out).all()
    assert np.abs(out.T.astype(np.float64) @ out - np.eye(r)).max() < 1e-5
    qx = _exact_qr(a)
    err = np.abs(out - qx).max(axis=0)
    rows = 4 if r <= 4 else (2 if r <= 8 else 1)     # powersgd.hip kOrthRows
    if n <= 1024 * rows:
        assert err.max() < 1e-5, err        # register-resident f64 MGS2: the exact factor
    else:                                   # tall: f32 storage between sweeps, still ahead of the reference
        ref_err = np.abs(O.orthogonalize(a) - qx).max(axis=0)
        assert np.all(err <= np.maximum(1e-5, ref_err)), (err, ref_err)


def test_orthogonalize_degenerate_columns():
    """A zero column (a layer whose gradient slice is zero): the reference's MGS divides 0 by 0 and
    the NaN spreads to every later column, then to P, Q and the decompressed gradient.  Here the
    zero column stays zero and the other columns are the exact factor.  An
    exactly repeated column: f32 rounding leaves a noise residual in both implementations; ours
    is still finite and orthonormal."""
    rng = np.random.default_rng(5)
    for n, r in ((4096, 4), (700, 3)):
        a = rng.standard_normal((n, r)).astype(np.float32)
        a[:, 1] = 0.0
        assert np.isnan(O.orthogonalize(a)).any()        # what the reference does
        out = _np(ops.orthogonalize_(_t(a)))
        assert np.isfinite(out).all()
        assert np.all(out[:, 1] == 0)
        keep = [c for c in range(r) if c != 1]
        assert np.abs(out[:, keep] - _exact_qr(a[:, keep])).max() < 1e-5
        a = rng.standard_normal((n, r)).astype(np.float32)
        a[:, 2] = a[:, 0]
        out = _np(ops.orthogonalize_(_t(a)))
        assert np.isfinite(out).all()
        assert np.abs(out.T.astype(np.float64) @ out - np.eye(r)).max() < 1e-5
        assert np.abs(out[:, :2] - _exact_qr(a[:, :2])).max() < 1e-5


def test_powersgd_compressor_golden(golden):
    from grace_amd.dist.compressor.powersgd import PowerSGDCompressor
    for c in golden.cases("powersgd", codec="powersgd"):
        if "steps" in c.meta:
            continue
        comp = PowerSGDCompressor(rank=c.meta["rank"], use_memory=True, world_size=1)
        comp.q_memory["w"] = _t(c["q0"])
        payload, ctx = comp.compress(_t(c["x"]), "w")
        p, q, shape = ctx
        m = int(np.prod(c["x"].shape[1:]))
        assert _close(_np(p), c["p"], m), c.name
        assert _close(_np(q), c["q"], m), c.name
        dec = _np(comp.decompress(payload, ctx))
        assert dec.shape == c["dec"].shape
        assert _close(dec, c["dec"], m), c.name


def test_powersgd_memory_allreduce_sequence(golden):
    """Two Allreduce(PowerSGD, PowerSGDMemory) steps with the reference's q draws injected."""
    from grace_amd.dist.communicator.allreduce import Allreduce
    from grace_amd.dist.compressor.powersgd import PowerSGDCompressor
    from grace_amd.dist.memory.powersgd import PowerSGDMemory
    c = golden.case("powersgd", "powersgd_memory_seq")
    comp = PowerSGDCompressor(rank=2, use_memory=True, world_size=1)
    mem = PowerSGDMemory(comp.q_memory, compress_rank=2)
    comm = Allreduce(comp, mem, 1)
    for s in range(2):
        g = _t(c[f"g{s}"])
        t = mem.compensate(g, "w")
        q0 = _t(c[f"qdraw{s}"])
        ops.orthogonalize_(q0)
        comp.q_memory["w"] = q0      # the reference drew and orthogonalised this q in compress
        payload, ctx = comp.compress(t, "w")
        mem.update(t, "w", comp, payload, ctx)
        out = comm.send_receive(payload, "w", ctx)
        # the stated bar: rel 1e-5 * sqrt(m), m = 40 columns
        m = c[f"g{s}"].shape[1]
        tscale = np.abs(c[f"t{s}"]).max()
        assert _close(_np(t), c[f"t{s}"], m), s
        assert _close(_np(ctx[0]), c[f"p{s}"], m), s
        assert _close(_np(ctx[1]), c[f"q{s}"], m), s
        assert _close(_np(out), c[f"dec{s}"], m, scale=tscale), s
        assert _close(_np(mem.residuals["w"]), c[f"res{s}"], m, scale=tscale), s


def test_one_dim_passthrough():
    from grace_amd.dist.compressor.powersgd import PowerSGDCompressor
    comp = PowerSGDCompressor(rank=4)
    x = _t(np.arange(10, dtype=np.float32))
    payload, ctx = comp.compress(x, "b")
    assert ctx is None and comp.decompress(payload, ctx) is x


@pytest.mark.parametrize("n,r", [(4096, 4), (5000, 3), (100, 1), (9000, 8), (300, 16)])
def test_orthogonalize_shapes_and_fused_draw(n, r):
    """Register-resident (n <= 4096) and chunked (taller) orthogonalisation against a float64
    MGS, and the fused draw == draw then orthogonalise."""
    rng = np.random.default_rng(n + r)
    a = rng.standard_normal((n, r)).astype(np.float32)
    out = _np(ops.orthogonalize_(_t(a)))
    exp = a.astype(np.float64)
    for i in range(r):
        exp[:, i] /= np.sqrt(np.sum(exp[:, i] ** 2))
        if i + 1 < r:
            exp[:, i + 1:] -= np.sum(exp[:, i:i + 1] * exp[:, i + 1:], axis=0) * exp[:, i:i + 1]
    assert np.allclose(out, exp, rtol=1e-4, atol=1e-5)
    fused = _np(ops.normal_orthogonal((n, r), 77, "cuda"))
    ref = _np(ops.orthogonalize_(ops.normal((n, r), 77, "cuda")))
    assert np.allclose(fused, ref, rtol=1e-5, atol=1e-6)
    assert np.allclose(fused.T.astype(np.float64) @ fused, np.eye(r), atol=1e-4)


@pytest.mark.parametrize("shape,r", [((4096, 4096), 4), ((256, 300), 4), ((100, 1000), 2), ((64, 48), 1), ((33, 17), 3)])
def test_p_with_q_drawn_in_the_contraction(shape, r):
    """grace_powersgd_p_draw == M @ normal((m, r), seed) (the grace_normal_fill stream), and the
    compressor's device path equals the reference's algorithm on that draw: orthogonalize(M q) with
    q = orthogonalize(draw) (powersgd.py:40-52) -- the same P, Q because orthogonalising q first only
    right-multiplies M q by an upper-triangular matrix."""
    from grace_amd.dist.compressor.powersgd import PowerSGDCompressor
    rng = np.random.default_rng(shape[0] * r)
    M = rng.standard_normal(shape).astype(np.float32)
    n, m = shape
    seed = 4242
    q0 = _np(ops.normal((m, r), seed, DEV))
    P = _np(ops.powersgd_p_draw(_t(M), r, seed))
    Pe = M.astype(np.float64) @ q0.astype(np.float64)
    assert _close(P, Pe, m)
    comp = PowerSGDCompressor(rank=r)
    payload, (p, q, shp) = comp.compress(_t(M), "w")
    seed_used = ops.step_seed("powersgd-q", "w", 1)
    q0 = _np(ops.normal((m, min(n, m, r)), seed_used, DEV))
    p_or, q_or = O.powersgd_compress(M, O.orthogonalize(q0))
    assert _close(_np(p), p_or, m, scale=1.0)
    assert _close(_np(q), q_or, m)
