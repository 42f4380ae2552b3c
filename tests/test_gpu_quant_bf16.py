"""QSGD and TernGrad on bfloat16 gradients at the level of grace_amd.ops.

The specification: codes, bucket norms and scalars are bit for bit what the f32 entry point gives for
the gradient widened to f32, and a dense result is the f32 result rounded once by torch's CPU
``.to(torch.bfloat16)`` (16-bit patterns; at NaN positions the pattern 0x7FC0).  Layer 1 pins the
bf16 entry points to the numpy oracle with injected uniforms (and injected norms / clamp bounds, as
tests/test_gpu_quant.py does for f32); layer 2 pins them to the f32 entry points with the device
generator, which is where the pipelined QSGD encoder runs; the last test repeats layer 2 on the
ResNet-50 set, the smallest input at which an encoder row runs more than one pipeline stage."""
import functools

import numpy as np
import pytest
import torch

from grace_amd import ops
from oracle import grace_oracle as O
from tests.golden_util import same_bits
from tests.test_gpu_topk_bf16 import _bits16, _np, check_dense

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16 = torch.bfloat16
# everything after the size-1 tensor starts on an odd element; 49155 = three TernGrad units + 3
SEG = (9408, 64, 64, 4096, 36864, 1, 129, 20480, 1000, 3, 49155)
SHAPES = [(1,), (127,), (128,), (129,), (4099,), (100003,), SEG]
KINDS = ("normal", "zero", "inf", "nan", "negzero")
CANARY = 0x7FFF   # a NaN pattern no kernel writes (a NaN result is 0x7FC0)


def _t(a):
    return torch.from_numpy(np.array(a)).to(DEV)    # (a copy: the cached inputs are read-only)


@functools.lru_cache(maxsize=None)
def _grad(sizes, kind):
    """(bf16 CPU tensor, its exact f32 upcast as a read-only array, injected uniforms)."""
    n = sum(sizes)
    g = np.random.default_rng(1000 + n + KINDS.index(kind))
    x = (g.standard_normal(n) * 0.01).astype(np.float32)
    offs = np.cumsum((0,) + sizes[:-1])
    big = int(offs[int(np.argmax(sizes))])          # the start of the largest tensor
    if kind == "zero":
        x[big:big + 128] = 0.0                       # an all-zero bucket (the whole tensor up to 128)
        if len(sizes) > 1:
            x[offs[2]:offs[2] + sizes[2]] = 0.0      # an all-zero tensor
    elif kind == "inf":
        x[big + min(70, sizes[int(np.argmax(sizes))] - 1)] = np.inf
    elif kind == "nan":
        x[big + (sizes[int(np.argmax(sizes))] - 1) // 2] = np.nan
    elif kind == "negzero":
        x[::7] = -0.0
    b = torch.from_numpy(x).to(BF16)
    up = b.float().numpy()
    up.setflags(write=False)
    u = g.random(n, dtype=np.float32)
    u.setflags(write=False)
    return b, up, u


def _segs(sizes, bucket=128):
    """(element offset, bucket offset, length, buckets) of every tensor"""
    off = noff = 0
    for n in sizes:
        nb = -(-n // bucket)
        yield off, noff, n, nb
        off, noff = off + n, noff + nb


def _same_bits_nan(a, b):
    """f32 arrays equal bit for bit, a NaN matching any NaN"""
    a, b = np.asarray(a, dtype=np.float32).ravel(), np.asarray(b, dtype=np.float32).ravel()
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and same_bits(a[~na], b[~nb])


def _int_bits(t):
    return t.view({1: torch.int8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def _equal_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_int_bits(a), _int_bits(b))


@pytest.fixture
def canary(monkeypatch):
    """Every bf16 device tensor torch.empty hands out during the test is pre-filled with CANARY; the
    returned check asserts that a result holds none, i.e. that it was written in full."""
    real = torch.empty

    def empty(*a, **kw):
        t = real(*a, **kw)
        if t.dtype == BF16 and t.is_cuda and t.numel():
            t.view(torch.int16).fill_(CANARY)
        return t
    monkeypatch.setattr(torch, "empty", empty)

    def written(out):
        assert out.dtype == BF16
        assert not bool((out.view(torch.int16) == CANARY).any()), "part of the bf16 result was not written"
        return out
    return written


def _nan_is_7fc0(out):
    nan = torch.isnan(out.float())
    assert bool((out.view(torch.int16)[nan] == 0x7FC0).all())


# ------------------------------------------------------------------------- 1. against the oracle
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("sizes", SHAPES, ids=lambda s: "n%d" % sum(s))
def test_qsgd_against_the_oracle(sizes, kind, canary):
    b, up, u = _grad(sizes, kind)
    xb, ud = b.to(DEV), _t(u)
    sz = list(sizes)
    for q in (127, 255):
        codes, norms = ops.qsgd_compress(xb, q, 128, sizes=sz, u=ud)
        assert codes.dtype == (torch.int8 if q < 128 else torch.float16) and norms.dtype == torch.float32
        cn, nn = _np(codes), _np(norms)
        exp_c, exp_d = [], []
        for off, noff, n, nb in _segs(sizes):
            ref_c, ref_n = O.qsgd_compress(up[off:off + n], u[off:off + n], q, 128)
            fin = np.isfinite(ref_n)
            # the device sums squares in f64, the reference in f32: within 4 ulp, NaN / inf where it has them
            assert np.array_equal(np.isfinite(nn[noff:noff + nb]), fin)
            assert ops.isclose_f32_ulps(nn[noff:noff + nb][fin], ref_n[fin], 4), (n, off)
            c, _ = O.qsgd_compress(up[off:off + n], u[off:off + n], q, 128, norms=nn[noff:noff + nb])
            exp_c.append(c)
            with np.errstate(invalid="ignore"):     # (inf norm times code 0)
                exp_d.append(O.qsgd_decode(c, nn[noff:noff + nb], q, 128, n))
        assert same_bits(cn, np.concatenate(exp_c)), q
        # injected norms are used as they are
        codes_i, norms_i = ops.qsgd_compress(xb, q, 128, sizes=sz, u=ud, norms_in=norms)
        assert _equal_bits(codes_i, codes) and _equal_bits(norms_i, norms)
        out = canary(ops.qsgd_step_w1(xb, q, sizes=sz, u=ud))
        check_dense(out, np.concatenate(exp_d))
        _nan_is_7fc0(out)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("sizes", SHAPES, ids=lambda s: "n%d" % sum(s))
def test_qsgd_cuda_variant_against_the_oracle(sizes, kind, canary):
    b, up, u = _grad(sizes, kind)
    xb, ud = b.to(DEV), _t(u)
    sz = list(sizes)
    codes, norms = ops.qsgd_compress(xb, 127, 128, sizes=sz, variant=1, u=ud)
    cn, nn = _np(codes), _np(norms)
    exp_d = np.empty(sum(sizes), dtype=np.float32)
    for off, noff, n, nb in _segs(sizes):
        x, uu = up[off:off + n], u[off:off + n]
        _, ref_n = O.qsgd_cuda_compress(x, uu, 127, 128)
        assert ops.isclose_f32_ulps(nn[noff:noff + nb], ref_n.astype(np.float32), 1), (n, off)
        exp_c, exp_n = O.qsgd_cuda_compress(x, uu, 127, 128, norms=nn[noff:noff + nb])
        assert np.array_equal(cn[off:off + n], exp_c), (n, off)
        d = ((exp_n.astype(np.float32)[np.arange(n) // 128] / np.float32(127)).astype(np.float32)
             * exp_c.astype(np.float32)).astype(np.float32)
        d[exp_c == -128] = np.nan
        exp_d[off:off + n] = d
    out = canary(ops.qsgd_step_w1(xb, 127, sizes=sz, variant=1, u=ud))
    check_dense(out, exp_d)
    _nan_is_7fc0(out)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("sizes", SHAPES, ids=lambda s: "n%d" % sum(s))
def test_terngrad_against_the_oracle(sizes, kind, canary):
    b, up, u = _grad(sizes, kind)
    xb, ud = b.to(DEV), _t(u)
    sz = list(sizes)
    segs = [(off, n) for off, _, n, _ in _segs(sizes)]
    clips = np.array([O.terngrad_clip(up[off:off + n]) for off, n in segs], dtype=np.float32)
    codes, scal = ops.terngrad_compress(xb, sizes=sz, clip=_t(clips), u=ud)
    assert codes.dtype == torch.int8 and scal.dtype == torch.float32
    with np.errstate(invalid="ignore"):     # (a NaN bound: the oracle casts NaN signs, replaced by 0 below)
        exp = [O.terngrad_compress(up[off:off + n], u[off:off + n], clip=clips[i]) for i, (off, n) in enumerate(segs)]
    exp_s = np.concatenate([e[1] for e in exp])
    assert _same_bits_nan(_np(scal), exp_s)
    exp_c = np.concatenate([e[0] if not np.isnan(e[1][0]) else np.zeros_like(e[0]) for e in exp])   # NaN scalar: all 0
    assert np.array_equal(_np(codes), exp_c)
    # the device's own bound (f64 sums, not the reference's f32 order) is NaN where the reference's is
    _, scal_d = ops.terngrad_compress(xb, sizes=sz, u=ud)
    assert np.array_equal(np.isnan(_np(scal_d)), np.isnan(exp_s))
    with np.errstate(invalid="ignore"):
        exp_d = np.concatenate([(c.astype(np.float32) * s[0]).astype(np.float32)
                                for c, s in ((exp_c[off:off + n], e[1]) for (off, n), e in zip(segs, exp))])
    out = canary(ops.terngrad_step_w1(xb, sizes=sz, clip=_t(clips), u=ud))
    check_dense(out, exp_d)
    _nan_is_7fc0(out)


# ----------------------------------------------------- 2. against the f32 entry points, device generator
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("sizes", SHAPES, ids=lambda s: "n%d" % sum(s))
def test_bf16_twins_equal_the_f32_entry_points(sizes, kind, canary):
    b, up, _ = _grad(sizes, kind)
    xb, xf = b.to(DEV), _t(up)
    sz, seed = list(sizes), 0xBF16 + sum(sizes)
    for q, variant in ((127, 0), (255, 0), (127, 1)):
        cb, nb = ops.qsgd_compress(xb, q, 128, sizes=sz, variant=variant, seed=seed)
        cf, nf = ops.qsgd_compress(xf, q, 128, sizes=sz, variant=variant, seed=seed)
        assert _equal_bits(cb, cf) and _equal_bits(nb, nf), (q, variant)
        out = canary(ops.qsgd_step_w1(xb, q, sizes=sz, variant=variant, seed=seed))
        ref = ops.qsgd_step_w1(xf, q, sizes=sz, variant=variant, seed=seed)
        assert ref.dtype == torch.float32 and out.shape == ref.shape
        check_dense(out, _np(ref))
        _nan_is_7fc0(out)
    cb, sb = ops.terngrad_compress(xb, sizes=sz, seed=seed)
    cf, sf = ops.terngrad_compress(xf, sizes=sz, seed=seed)
    assert _equal_bits(cb, cf) and _equal_bits(sb, sf)
    out = canary(ops.terngrad_step_w1(xb, sizes=sz, seed=seed))
    check_dense(out, _np(ops.terngrad_step_w1(xf, sizes=sz, seed=seed)))
    _nan_is_7fc0(out)


@pytest.mark.parametrize("world", [1, 2, 5])
@pytest.mark.parametrize("sizes", [(129,), (4099,), SEG], ids=lambda s: "n%d" % sum(s))
def test_decode_aggregate_rounds_the_f32_result_once(sizes, world, canary):
    """W rank-major payloads (every kind of value among the ranks), with and without the Python-sum
    zero, divisors W and 1; the 4099-element tensor gives a code stride that is no multiple of 4."""
    n, sz = sum(sizes), list(sizes)
    ups = [_t(_grad(sizes, KINDS[w % len(KINDS)])[1]) for w in range(world)]
    for q, variant in ((127, 0), (255, 0), (127, 1)):
        pay = [ops.qsgd_compress(x, q, 128, sizes=sz, variant=variant, seed=77 + w) for w, x in enumerate(ups)]
        codes, norms = torch.cat([p[0] for p in pay]), torch.cat([p[1] for p in pay])
        for aggregate in (False, True):
            for divisor in sorted({1.0, float(world)}):
                kw = dict(sizes=sz, variant=variant, world=world, aggregate=aggregate, divisor=divisor)
                out = canary(ops.qsgd_decompress(codes, norms, q, 128, n, out_dtype=BF16, **kw))
                check_dense(out, _np(ops.qsgd_decompress(codes, norms, q, 128, n, **kw)))
                _nan_is_7fc0(out)
    pay = [ops.terngrad_compress(x, sizes=sz, seed=77 + w) for w, x in enumerate(ups)]
    codes, scal = torch.cat([p[0] for p in pay]), torch.cat([p[1] for p in pay])
    for aggregate in (False, True):
        for divisor in sorted({1.0, float(world)}):
            kw = dict(sizes=sz, world=world, aggregate=aggregate, divisor=divisor)
            out = canary(ops.terngrad_decompress(codes, scal, n, out_dtype=BF16, **kw))
            check_dense(out, _np(ops.terngrad_decompress(codes, scal, n, **kw)))
            _nan_is_7fc0(out)


def test_f32_calls_are_unchanged_and_results_are_new_tensors():
    """out_dtype defaults to float32, a step returns its input's dtype and never its storage."""
    b, up, _ = _grad((4099,), "normal")
    xb, xf = b.to(DEV), _t(up)
    for x in (xb, xf):
        for out in (ops.qsgd_step_w1(x, 127, seed=3), ops.terngrad_step_w1(x, seed=3)):
            assert out.dtype == x.dtype and out.shape == x.shape and out.data_ptr() != x.data_ptr()
    codes, norms = ops.qsgd_compress(xb, 127, 128, seed=3)
    assert ops.qsgd_decompress(codes, norms, 127, 128, 4099).dtype == torch.float32
    tc, ts = ops.terngrad_compress(xb, seed=3)
    assert ops.terngrad_decompress(tc, ts, 4099).dtype == torch.float32
    with pytest.raises(ValueError):     # a view that starts on an odd element is not 8-byte aligned
        ops.qsgd_step_w1(torch.zeros(4100, dtype=BF16, device=DEV)[1:], 127)


# ------------------------------------------------------------------------- 3. the ResNet-50 set
def test_resnet50_set_bf16_equals_f32(canary):
    """161 tensors, 199,672 buckets: more than 4096 x 32, so rows of the pipelined QSGD encoder run
    several stages and the prefetch of the next stage is exercised."""
    import bench
    sizes = [int(np.prod(s)) for s in bench.resnet50_shapes()]
    assert len(sizes) == 161 and sum(-(-s // 128) for s in sizes) == 199672 > 4096 * 32
    n = sum(sizes)
    xb = (torch.randn(n, device=DEV, generator=torch.Generator(DEV).manual_seed(5)) * 0.01).to(BF16)
    xf = xb.float()
    cb, nb = ops.qsgd_compress(xb, 127, 128, sizes=sizes, seed=11)
    cf, nf = ops.qsgd_compress(xf, 127, 128, sizes=sizes, seed=11)
    assert _equal_bits(cb, cf) and _equal_bits(nb, nf)
    out = canary(ops.qsgd_step_w1(xb, 127, sizes=sizes, seed=11))
    ref = ops.qsgd_step_w1(xf, 127, sizes=sizes, seed=11)
    assert np.array_equal(_bits16(out), _bits16(ref.cpu().to(BF16)))
    cb, sb = ops.terngrad_compress(xb, sizes=sizes, seed=11)
    cf, sf = ops.terngrad_compress(xf, sizes=sizes, seed=11)
    assert _equal_bits(cb, cf) and _equal_bits(sb, sf)
    out = canary(ops.terngrad_step_w1(xb, sizes=sizes, seed=11))
    ref = ops.terngrad_step_w1(xf, sizes=sizes, seed=11)
    assert np.array_equal(_bits16(out), _bits16(ref.cpu().to(BF16)))
