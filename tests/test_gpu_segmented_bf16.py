"""bfloat16 gradients through the segmented per-tensor top-k (grace_amd/csrc/topk.hip "Segmented",
element type uint16_t; grace_amd.segmented_bf16.SegmentedTopK) and the DDP harness's GradBucket.

The specification is DESIGN.md §9's, per tensor: every result is what the f32 segmented step gives for
the gradient widened to f32.  So the payload (global indices), the f32 residual and the f32 dense
result come from ``oracle.grace_oracle`` run per tensor on the upcast gradient, bit for bit, and the
bf16 dense result is that f32 result rounded as torch's CPU cast rounds (check_dense of
tests/test_gpu_topk_bf16.py).  Gradients are drawn in f32 from a seed and rounded to bf16 by torch
on the CPU; every planted value (0.5, 1000.0, +-inf, -0) is exact in bf16.  Each reference is
computed once and shared read-only by the tests that use it."""
import functools

import numpy as np
import pytest
import torch

from oracle import grace_oracle as O
from tests.golden_util import same_bits
from tests.test_gpu_harness import _sample_positions
from tests.test_gpu_topk_bf16 import check_dense

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
RATIO = 0.01
# test_segmented_edge_segments' list plus one segment longer than three 32768-element chunks: small
# segments, the 8192 / 8193 boundary, large ones below one chunk, and several chunks plus a tail at both
# bf16 chunk lengths (20480 with a residual stream, 32768 without).  The 50001, 60000 and 33000 segments
# start at multiples of 4 (full chunks on the vector path), 20000 and 131075 at 2 mod 4 and 65536 and
# 8193 at odd offsets (the guarded path)
EDGE_SIZES = (3, 40000, 5, 50001, 65536, 7, 60000, 33000, 1, 8193, 20000, 8192, 131075)
FACTOR_SIZES = (9000, 70000, 5, 33001)


def _frozen(a):
    a.setflags(write=False)
    return a


def edge_grads(seed, step):
    """One step's per-tensor gradients over EDGE_SIZES, as f32 arrays holding bf16 values."""
    rng = np.random.default_rng([seed, step])
    gs = [rng.standard_normal(n).astype(np.float32) for n in EDGE_SIZES]
    gs[1][:] = np.float32(0.5)                                     # all ties
    gs[3][[0, 7, 77, 777, 50000]] = [np.nan, np.inf, -np.inf, -0.0, np.nan]
    g2 = rng.random(65536).astype(np.float32) - np.float32(0.5)
    free = np.setdiff1d(np.arange(65536), _sample_positions(65536))
    g2[free[rng.permutation(free.size)[:3 * 655]]] = np.float32(1000.0)
    gs[4] = g2                                                     # the sampled bracket misses
    z = np.zeros(60000, np.float32)
    z[rng.permutation(60000)[:60]] = rng.standard_normal(60).astype(np.float32)
    gs[6] = z                                                      # mostly zeros: the k-th key is 0
    return [_frozen(torch.from_numpy(g).to(BF16).float().numpy()) for g in gs]


def reference(grads, ratio=RATIO, beta=1.0, gamma=1.0):
    """grads[step][tensor] (f32 arrays) -> per step a list of the oracle's (vals, idx, residual, out)
    per tensor, the residuals carried from step to step."""
    res = [None] * len(grads[0])
    steps = []
    for gs in grads:
        row = []
        for j, g in enumerate(gs):
            _, v, i, res[j], out = O.topk_residual_step(g, res[j], ratio, beta=beta, gamma=gamma)
            row.append((_frozen(v), _frozen(i), _frozen(res[j]), _frozen(out)))
        steps.append(row)
    return steps


@functools.lru_cache(maxsize=None)
def _edge_case():
    grads = [edge_grads(31, s) for s in range(3)]
    return grads, reference(grads)


@functools.lru_cache(maxsize=None)
def _factor_case():
    rng = np.random.default_rng(47)
    grads = [[_frozen(torch.from_numpy(rng.standard_normal(n).astype(np.float32)).to(BF16).float().numpy())
              for n in FACTOR_SIZES] for _ in range(3)]
    return grads, reference(grads, beta=0.9, gamma=0.5)


def _flat_bf16(gs, offset=0):
    """The tensors back to back as one bf16 device buffer; offset: a view that many elements into
    its allocation."""
    cat = torch.from_numpy(np.concatenate(gs)).to(BF16)
    buf = torch.empty(cat.numel() + offset, dtype=BF16, device="cuda")
    flat = buf[offset:]
    flat.copy_(cat)
    assert flat.data_ptr() == buf.data_ptr() + 2 * offset
    return flat


def check_step(eng, sizes, exp, out, name="bucket", where=()):
    """The engine's payload and residual after a step, and its dense result `out` (bf16 or f32
    tensor, or None), against the per-tensor reference row `exp`."""
    vals, idx = (t.cpu().numpy() for t in eng.last_payload)
    idx = idx.astype(np.int64)
    r = eng.residuals[name]
    assert r.dtype == torch.float32 and vals.dtype == np.float32 and eng.last_payload[1].dtype == torch.int32
    rcat = r.cpu().numpy()
    if out is not None and out.dtype == torch.float32:
        out_np = out.cpu().numpy()
    off = koff = 0
    for j, n in enumerate(sizes):
        v_or, i_or, r_or, o_or = exp[j]
        if out is not None and out.dtype == BF16:
            check_dense(out[off:off + n], o_or)
        elif out is not None:
            assert same_bits(out_np[off:off + n], o_or), (*where, j)
        k = i_or.size
        mine = idx[koff:koff + k] - off
        order = np.argsort(mine)
        assert np.array_equal(mine[order], i_or.astype(np.int64)), (*where, j)
        assert same_bits(vals[koff:koff + k][order], v_or), (*where, j)
        assert same_bits(rcat[off:off + n], r_or), (*where, j)
        off += n
        koff += k
    assert koff == idx.size


# ------------------------------------------------------------------------------- 1. edge segments
@pytest.mark.parametrize("world", [1, 2])
def test_edge_segments(world):
    """Three steps (the first without a residual, then with one and a live carry) over EDGE_SIZES:
    world 1 with the bf16 dense result, world 2's local half (residual and payload only)."""
    from grace_amd.segmented_bf16 import SegmentedTopK
    grads, ref = _edge_case()
    eng = SegmentedTopK(RATIO, world_size=world)
    for s, gs in enumerate(grads):
        flat = _flat_bf16(gs)
        before = flat.clone()
        if world == 1:
            out = eng.step(flat, EDGE_SIZES)
            assert out.dtype == BF16 and out.data_ptr() != flat.data_ptr()
        else:
            eng.local_step(flat, EDGE_SIZES)
            out = None
        assert torch.equal(flat.view(torch.int16), before.view(torch.int16))   # the gradient is only read
        check_step(eng, EDGE_SIZES, ref[s], out, where=(world, s))
    assert eng._carries["bucket"][0].dtype == torch.float32


# ------------------------------------------------------------------------------- 2. in place
def test_in_place_equals_out_of_place():
    """out = flat, as harness.step_segmented runs it: bit for bit the out-of-place result."""
    from grace_amd.segmented_bf16 import SegmentedTopK
    grads, ref = _edge_case()
    eng, eng_in = SegmentedTopK(RATIO), SegmentedTopK(RATIO)
    for s, gs in enumerate(grads):
        out = eng.step(_flat_bf16(gs), EDGE_SIZES)
        flat = _flat_bf16(gs)
        got = eng_in.step(flat, EDGE_SIZES, out=flat)
        assert got is flat
        check_step(eng_in, EDGE_SIZES, ref[s], flat, where=("in place", s))
        nan = torch.isnan(out.float())
        assert torch.equal(torch.isnan(flat.float()), nan)
        assert torch.equal(flat.view(torch.int16)[~nan], out.view(torch.int16)[~nan])
        assert torch.equal(eng_in.residuals["bucket"].view(torch.int32), eng.residuals["bucket"].view(torch.int32))


# ------------------------------------------------------------------------------- 3. factors
def test_factors():
    from grace_amd.segmented_bf16 import SegmentedTopK
    grads, ref = _factor_case()
    eng = SegmentedTopK(RATIO)
    eng.beta, eng.gamma = 0.9, 0.5
    for s, gs in enumerate(grads):
        out = eng.step(_flat_bf16(gs), FACTOR_SIZES)
        check_step(eng, FACTOR_SIZES, ref[s], out, where=("factors", s))


# ------------------------------------------------------------------------------- 4. unaligned base
def test_unaligned_base():
    """The gradient one bf16 element (2 bytes) into its allocation: every segment takes the guarded
    path, with the same results."""
    from grace_amd.segmented_bf16 import SegmentedTopK
    grads, ref = _edge_case()
    eng = SegmentedTopK(RATIO)
    for s, gs in enumerate(grads):
        flat = _flat_bf16(gs, offset=1)
        assert flat.data_ptr() % 4 == 2
        out = eng.step(flat, EDGE_SIZES)
        check_step(eng, EDGE_SIZES, ref[s], out, where=("unaligned", s))


# ------------------------------------------------------------------------------- 5. dtype switch
def test_dtype_switch_keeps_residual_and_carry():
    """One name stepped f32, bf16, f32: the f32 residual and the carry stay the same tensors and
    every step follows the oracle on the upcast gradient."""
    from grace_amd.segmented_bf16 import SegmentedTopK
    rng = np.random.default_rng(53)
    grads = [[rng.standard_normal(n).astype(np.float32) for n in FACTOR_SIZES] for _ in range(3)]
    grads[1] = [torch.from_numpy(g).to(BF16).float().numpy() for g in grads[1]]
    ref = reference(grads)
    eng = SegmentedTopK(RATIO)
    kept = None
    for s, gs in enumerate(grads):
        flat = _flat_bf16(gs) if s == 1 else torch.from_numpy(np.concatenate(gs)).cuda()
        out = eng.step(flat, FACTOR_SIZES, "w")
        assert out.dtype == flat.dtype
        check_step(eng, FACTOR_SIZES, ref[s], out, name="w", where=("switch", s))
        now = (eng.residuals["w"], eng._carries["w"][0])
        assert kept is None or (now[0] is kept[0] and now[1] is kept[1])
        kept = now


# ------------------------------------------------------------------------------- 6. f32 unmoved
def test_f32_path_unmoved():
    from grace_amd.segmented_bf16 import SegmentedTopK
    rng = np.random.default_rng(59)
    grads = [[rng.standard_normal(n).astype(np.float32) for n in FACTOR_SIZES] for _ in range(2)]
    ref = reference(grads)
    eng = SegmentedTopK(RATIO)
    for s, gs in enumerate(grads):
        out = eng.step(torch.from_numpy(np.concatenate(gs)).cuda(), FACTOR_SIZES)
        assert out.dtype == torch.float32
        check_step(eng, FACTOR_SIZES, ref[s], out, where=("f32", s))


# ------------------------------------------------------------------------------- 7. refusals
def test_refusals():
    from grace_amd.segmented_bf16 import SegmentedTopK
    sizes = [100, 9000]
    eng = SegmentedTopK(RATIO)
    with pytest.raises(TypeError):
        eng.step(torch.zeros(9100, dtype=torch.float16, device="cuda"), sizes)
    g = torch.zeros(9100, dtype=BF16, device="cuda")
    with pytest.raises(TypeError):
        eng.step(g, sizes, out=torch.empty(9100, dtype=torch.float32, device="cuda"))
    with pytest.raises(TypeError):
        eng.local_step(g, sizes, dense=torch.empty(9100, dtype=torch.float32, device="cuda"))
    with pytest.raises(TypeError):
        SegmentedTopK(RATIO, world_size=2).step(g, sizes, out=torch.empty(9100, dtype=torch.float32, device="cuda"))
    # an unusable result buffer is refused before the step touches the name's residual, at any world
    for world in (1, 2):
        e = SegmentedTopK(RATIO, world_size=world)
        with pytest.raises(ValueError):
            e.step(g, sizes, out=torch.empty(9101, dtype=BF16, device="cuda"))
        with pytest.raises(ValueError):
            e.step(g, sizes, out=torch.empty(18200, dtype=BF16, device="cuda")[::2])
        assert not e.residuals and not e._carries


# ------------------------------------------------------------------------------- 8. harness
def test_harness_bucket_over_a_bf16_model():
    """GradBucket over a bf16 model: a bf16 flat buffer whose views are the parameters' .grad, and
    step_segmented leaves every tensor's result in them (no backward is run: this is about the
    bucket and the engine)."""
    from grace_amd.segmented_bf16 import SegmentedTopK
    from grace_amd.harness import GradBucket, ShapeModel, step_segmented
    shapes = [(64,), (100, 80), (300, 200), (8192,), (41, 1000), (3,)]
    sizes = [int(np.prod(s)) for s in shapes]
    assert min(sizes) <= 8192 < 32768 < max(sizes)
    model = ShapeModel(shapes, "cuda").to(BF16)
    bucket = GradBucket(model)
    assert bucket.flat.dtype == BF16 and bucket.sizes == sizes
    offs = np.cumsum([0] + sizes)
    for p, o in zip(bucket.params, offs):
        assert p.grad.dtype == BF16 and p.grad.shape == p.shape and p.grad.data_ptr() == bucket.flat[int(o):].data_ptr()
    rng = np.random.default_rng(61)
    grads = [[torch.from_numpy(rng.standard_normal(n).astype(np.float32)).to(BF16).float().numpy() for n in sizes]
             for _ in range(2)]
    ref = reference(grads)
    eng = SegmentedTopK(RATIO)
    for s, gs in enumerate(grads):
        bucket.flat.copy_(torch.from_numpy(np.concatenate(gs)).to(BF16))
        step_segmented(bucket, eng)
        check_step(eng, sizes, ref[s], bucket.flat, where=("harness", s))
        for j, p in enumerate(bucket.params):
            check_dense(p.grad.reshape(-1), ref[s][j][3])


def test_harness_bucket_refuses_mixed_dtypes():
    from grace_amd.harness import GradBucket, ShapeModel
    model = ShapeModel([(10,), (20,)], "cuda")
    model.ps[1].data = model.ps[1].data.to(BF16)
    with pytest.raises(TypeError):
        GradBucket(model)
    f32 = GradBucket(ShapeModel([(10,), (20,)], "cuda"))
    assert f32.flat.dtype == torch.float32 and f32.flat.numel() == 30


# ------------------------------------------------------------------------------- 9. decode into a buffer
@pytest.mark.parametrize("dtype", [torch.float32, BF16])
def test_sparse_aggregate_sorted_into_a_buffer(dtype):
    """ops.sparse_aggregate_sorted(out=): the caller's buffer (filled with a sentinel first: the
    decode writes every element) equals the allocated result; a wrong dtype or size is refused."""
    from grace_amd import ops
    n, k, world = 20000, 300, 2          # two full 8192-element chunks and a guarded tail
    rng = np.random.default_rng(67)
    pays = []
    for _ in range(world):
        idx = np.sort(rng.choice(n, k, replace=False)).astype(np.int32)
        vals = rng.standard_normal(k).astype(np.float32)
        pay = torch.from_numpy(np.concatenate([vals, idx.view(np.float32)])).cuda()
        pays.append(ops.sort_payload(pay, k, n))
    gathered = torch.cat(pays)
    exp = ops.sparse_aggregate_sorted(gathered, k, world, n, world, out_dtype=dtype)
    buf = torch.full((n,), 7.0, dtype=dtype, device="cuda")
    got = ops.sparse_aggregate_sorted(gathered, k, world, n, world, out_dtype=dtype, out=buf)
    assert got is buf and got.dtype == dtype
    assert torch.equal(got, exp) and int((exp != 0).sum()) > k
    other = BF16 if dtype == torch.float32 else torch.float32
    with pytest.raises(ValueError):
        ops.sparse_aggregate_sorted(gathered, k, world, n, world, out_dtype=dtype,
                                    out=torch.empty(n, dtype=other, device="cuda"))
    with pytest.raises(ValueError):
        ops.sparse_aggregate_sorted(gathered, k, world, n, world, out_dtype=dtype,
                                    out=torch.empty(n + 1, dtype=dtype, device="cuda"))
