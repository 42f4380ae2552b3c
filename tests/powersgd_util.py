"""Helpers of the PowerSGD branch tests (tests/test_gpu_powersgd_branches.py): the componentwise
dot-product bound, and the launch choices of grace_amd/csrc/powersgd.hip restated from its constants
so that every case can assert which kernel path it runs."""
import numpy as np

U32 = 2.0 ** -24          # unit roundoff of float32 (round to nearest)


def dot_bound(A, B, k):
    """Componentwise bound on |fl(A @ B) - A @ B| for length-k f32 dot products summed in ANY order:
    Higham's gamma_k |A| |B| with gamma_k ~ k u (Accuracy and Stability of Numerical Algorithms,
    section 3.1), doubled because the rounding of the MFMA's internal 4-term accumulation is not
    documented."""
    return 2 * k * U32 * (np.abs(np.asarray(A, dtype=np.float64)) @ np.abs(np.asarray(B, dtype=np.float64)))


def project_close(a, b, k, scale=None):
    """The project's bar: rel 1e-5 * sqrt(k), absolute part on the global scale."""
    tol = 1e-5 * np.sqrt(k)
    scale = np.abs(b).max() if scale is None else scale
    return bool(np.allclose(a, b, rtol=tol, atol=tol * max(scale, 1e-30)))


# The constants and launch arithmetic below restate grace_amd/csrc/powersgd.hip:1675-1706 (p_ksplit,
# qt_slab, qt4_ok, qt4_slab) and the launchers after them (launch_p, grace_powersgd_qt).  A retune
# there that moves a boundary makes the branch asserted for a case differ: the table then fails
# instead of quietly no longer covering the path.
K_TILE_R = 16
TILE_C = 256
K_FAN = 8
K_TICKETS = 65536
K_Q4C = 1024
K_Q4D = 16
K_QT_WG = 1024
K_QT4_WG = 256
K_KSPLIT_MAX = 64


def _cdiv(a, b):
    return (a + b - 1) // b


def p_launch(n, m, r, m_aligned=True, qp_aligned=True):
    """launch_p's choice: kernel "r4" (VEC, R4), "vec" (VEC, generic) or "scalar" (no 16-B loads of
    M), the K split, how many of its chunks hold no tile, and whether the row tiles outnumber the
    tickets (then no split)."""
    vec = m % 4 == 0 and m_aligned
    r4 = r == 4 and qp_aligned and n * 16 * 64 < 2 ** 31
    tiles = _cdiv(n, K_TILE_R)
    nkt = _cdiv(m, TILE_C)
    ks = 1 if tiles > K_TICKETS else max(1, min(_cdiv(2048, tiles), nkt, K_KSPLIT_MAX))
    per = _cdiv(nkt, ks)
    return {"kernel": "r4" if vec and r4 else ("vec" if vec else "scalar"), "r4": r4, "ksplit": ks,
            "per": per, "empty": ks - _cdiv(nkt, per), "over_tickets": tiles > K_TICKETS}


def _qt_slabs(n, m):
    """qt_slab: (slab count before the doubling loop, after it, whether one slab takes every row
    because the column groups alone would outnumber the tickets)."""
    groups = _cdiv(m, TILE_C)
    if groups * 128 > K_TICKETS // 2:
        return 1, 1, True
    slab = max(_cdiv(_cdiv(n, _cdiv(K_QT_WG, groups)), K_TILE_R) * K_TILE_R, 2 * K_TILE_R)
    before = _cdiv(n, slab)
    while _cdiv(n, slab) > 16 * K_FAN:
        slab *= 2
    return before, _cdiv(n, slab), False


def _qt4_ok(m):
    return _cdiv(m, K_Q4C) * 16 <= K_TICKETS // 2


def _qt4_slabs(n, m):
    """qt4_slab: slab count before and after the doubling loop."""
    slab = _cdiv(_cdiv(n, _cdiv(K_QT4_WG, _cdiv(m, K_Q4C))), 4 * K_Q4D) * 4 * K_Q4D
    before = _cdiv(n, slab)
    while _cdiv(n, slab) > 16 * K_FAN:
        slab *= 2
    return before, _cdiv(n, slab)


def qt_launch(n, m, r, m_aligned=True, p_aligned=True):
    """grace_powersgd_qt's choice: kernel "qt4", "vec" or "scalar"; the slab count before and after
    the doubling loop; and qt_reduce_slabs' path: "single" (one slab), else "v4" or "scalar" partials
    with one or two levels and the size of the last group of kFan slabs."""
    vec = m % 4 == 0 and m_aligned
    qt4 = r == 4 and vec and _qt4_ok(m) and p_aligned
    if qt4:
        groups, whole_n = _cdiv(m, K_Q4C), False
        before, nslab = _qt4_slabs(n, m)
    else:
        groups = _cdiv(m, TILE_C)
        before, nslab, whole_n = _qt_slabs(n, m)
    out = {"kernel": "qt4" if qt4 else ("vec" if vec else "scalar"), "groups": groups, "slabs_before": before,
           "nslab": nslab, "whole_n": whole_n}
    if nslab == 1:
        out["reduce"] = "single"
    else:
        # 16-B partials: whole quads per slab run, 32-bit byte offsets (Q and the partials are 16-B aligned)
        v4 = (m * r) % 4 == 0 and m * r * 4 * max(K_FAN, _cdiv(nslab, K_FAN)) < 2 ** 31
        out["reduce"] = "v4" if v4 else "scalar"
        out["levels"] = 1 if nslab <= K_FAN else 2
        out["last_group"] = nslab - (_cdiv(nslab, K_FAN) - 1) * K_FAN
    return out


def workspace_bytes(n, m, r):
    """grace_powersgd_workspace_bytes: the tickets, then the larger of P's K-chunk partials and Qt's
    slab partials (both levels).  The library's figure is the one place its launch arithmetic can be
    read back, so the tests compare it with this restatement: a retune of p_ksplit / qt_slab /
    qt4_slab that this file does not follow shows up there."""
    pp = 4 * p_launch(n, m, r)["ksplit"] * n * r
    nslab = _qt_slabs(n, m)[1]
    if r == 4 and _qt4_ok(m):
        nslab = max(nslab, _qt4_slabs(n, m)[1])
    qp = 4 * (nslab + _cdiv(nslab, K_FAN)) * m * r
    return 4 * K_TICKETS + _cdiv(max(pp, qp), 256) * 256


def orth_rows(r):
    """psgd_orth_kernel's register-resident limit: kOrthBlock (1024) threads x kOrthRows rows."""
    return 1024 * (4 if r <= 4 else (2 if r <= 8 else 1))


def misaligned(t):
    """A dense copy of device tensor t that starts 4 bytes into a 16-B aligned buffer."""
    import torch
    buf = torch.empty(t.numel() + 8, dtype=t.dtype, device=t.device)
    assert buf.data_ptr() % 16 == 0
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v
