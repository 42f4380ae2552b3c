"""DGC on bfloat16 gradients at world size 1 (grace_amd.dgc_bf16.DgcCompressor, the ``_bf16`` entry
points of include/grace_hip_dgc.h) against the oracle on the widened gradient: ``out`` is the f32
result rounded once (tests/shard_select_util.round_cpu), ``r``, ``a`` and the meta's threshold and
count are the f32 step's, everything bit for bit.  ``rng="torch_cpu"`` with the reference's sample
stream replayed, or injected sample indices, throughout."""
import numpy as np
import pytest
import torch

from grace_amd import _lib, ops
from oracle import grace_oracle as O
from tests.dgc_bf16_util import LOOP_PATH_HOLDS, bf16_pair, rounded_case
from tests.dgc_edge_util import LOOP_CASES, bits, ns_of
from tests.golden_util import same_bits
from tests.shard_select_util import round_cpu

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = np.float32
BF16 = torch.bfloat16
RATIO, MOM, STEPS = 0.01, 0.9, 3
# 1 and 7: the scalar loop only; 16384: exactly one workgroup of the speculative pass; 16389: a tail
# in a second workgroup; 40000: the edge cases' size; 49154: three workgroups and two elements
SHAPES = [1, 7, 16384, 16389, 40000, 49154]


def _np(t):
    return t.detach().cpu().numpy()


def _out_bits(out):
    assert out.dtype == BF16
    return _np(out.contiguous().view(torch.int16)).ravel()


def _want_bits(out32):
    return round_cpu(torch.from_numpy(np.ascontiguousarray(out32))).numpy().astype(np.uint16).view(np.int16).ravel()


def _meta(slot="dgc_w1"):
    """{thr0, thr, count, nan0, fix} of a DGC workspace's meta words."""
    w = _np(ops.workspace(slot, 1, torch.device(DEV, torch.cuda.current_device()))[:20].view(torch.int32))
    return w.view(np.uint32)


def _grad(n, seed, specials=True):
    """(bf16 device tensor, its f32 widening): Gaussian with NaN, +-inf, -0 and bf16 subnormals."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(n).astype(F32)
    if specials and n >= 7:
        at = rng.choice(n, min(n, 12), replace=False)
        x[at[0]] = -0.0
        x[at[1]] = F32(3e-39)                     # a bf16 subnormal (and an f32 one)
        x[at[2]] = F32(-9.2e-41)                  # the smallest bf16 subnormal's neighbourhood
        if n >= 16384:
            x[at[3]], x[at[4]], x[at[5]] = np.inf, -np.inf, np.nan
            x[at[6:]] = -0.0
    b, w = bf16_pair(x)
    return b.to(DEV), w


def _oracle_step(g, r, a, sidx, ratio=RATIO, momentum=MOM):
    """Allgather(DgcCompressor, DgcMemory, 1).step on the CPU; r = a = None on a name's first step."""
    with np.errstate(invalid="ignore", over="ignore"):
        t, rc, ac = O.dgc_memory_compensate(g, r, a, momentum)
        vals, idx, mask, thr = O.dgc_compress(t, sidx, ratio)
        rn, an = O.dgc_memory_update(rc, ac, mask)
        out = (O.python_sum([O.sparse_decode(vals, idx, t.size)]) / F32(1)).astype(F32)
    return dict(out=out, r=rn, a=an, thr=thr, total=int(idx.size), path=O.dgc_adjust_path(t, sidx, ratio))


def _check_meta(e, what, slot="dgc_w1"):
    m = _meta(slot)
    if np.isnan(e["thr"]):
        assert np.isnan(m[1:2].view(F32)[0]), what
    else:
        assert int(m[1]) == bits(e["thr"]), (what, hex(int(m[1])), hex(bits(e["thr"])))
    assert int(m[2]) == e["total"], (what, int(m[2]), e["total"])


def _draw(n, seed):
    """The sample indices DgcCompressor(rng='torch_cpu') draws after torch.manual_seed(seed)."""
    torch.manual_seed(seed)
    return torch.empty([ns_of(n)]).uniform_(0, n).type(torch.long).numpy()


def _comm(cls, clipping=False):
    from grace_amd.dist.communicator.allgather import Allgather
    from grace_amd.dist.memory.dgc import DgcMemory
    return Allgather(cls(RATIO, rng="torch_cpu"), DgcMemory(MOM, clipping, 1), 1)


def _classes():
    from grace_amd.dgc_bf16 import DgcCompressor
    from grace_amd.dist.compressor.dgc import DgcCompressor as Parent
    return DgcCompressor, Parent


# ------------------------------------------------------------------------------- the fused step
@pytest.mark.parametrize("n", SHAPES)
def test_fused_step_shapes_three_steps_vs_oracle(n):
    """has_state false, then true twice, with the momentum state carried; special values in g."""
    comm = _comm(_classes()[0])
    r = a = None
    for s in range(STEPS):
        gb, gw = _grad(n, 100 * n + s)
        sidx = _draw(n, 50 + s)
        e = _oracle_step(gw, r, a, sidx)
        torch.manual_seed(50 + s)
        out = comm.step(gb.view(1, n), "w")
        assert out.dtype == BF16 and out.shape == (1, n)
        assert np.array_equal(_out_bits(out), _want_bits(e["out"])), (n, s)
        rd, ad = comm.memory.residuals["w"], comm.memory.gradients["w"]
        assert rd.dtype == ad.dtype == torch.float32
        assert same_bits(_np(rd), e["r"]) and same_bits(_np(ad), e["a"]), (n, s)
        _check_meta(e, (n, s))
        r, a = e["r"], e["a"]


def _raw_fused(gb, r, a, has, sidx, g_off, st_off):
    """grace_dgc_step_w1_fused_bf16 on views that start g_off bf16 elements (g, out) and st_off f32
    elements (the old and the new state) into 16-byte aligned buffers."""
    n = gb.numel()

    def at(src, off, dtype):
        buf = torch.empty(n + 8, dtype=dtype, device=DEV)
        assert buf.data_ptr() % 16 == 0
        v = buf[off:off + n]
        if src is not None:
            v.copy_(src)
        return v
    g = at(gb, g_off, BF16)
    out = at(None, g_off, BF16)
    ro, ao = at(None, st_off, torch.float32), at(None, st_off, torch.float32)
    ri = at(r, st_off, torch.float32) if has else None
    ai = at(a, st_off, torch.float32) if has else None
    top, kt = ops._dgc_sample_top_of(g, RATIO, sidx, 0, state=(ri, ai, has, MOM))
    ws = ops.workspace("dgc_w1", _lib.query("grace_dgc_step_w1_fused_workspace_bytes", n), g.device)
    _lib.call("grace_dgc_step_w1_fused_bf16", g.data_ptr(), ri.data_ptr() if has else None,
              ai.data_ptr() if has else None, 1 if has else 0, MOM, n, top.data_ptr(), kt, RATIO, ws.data_ptr(),
              ro.data_ptr(), ao.data_ptr(), out.data_ptr(), ops._stream())
    return out, ro, ao


@pytest.mark.parametrize("sample", ["kth", "largest"])           # thr0 stands / the gated fix-up runs
@pytest.mark.parametrize("has", [False, True])
def test_fused_step_misaligned_views_equal_aligned(has, sample):
    """g and out 1, 2 and 4 elements into a larger buffer (2, 4 and 8 bytes off 16), the f32 state
    1 and 2 elements in: the scalar loops give what the vector path gives."""
    n = 40000
    gb, gw = _grad(n, 7)
    rng = np.random.default_rng(8)
    r = torch.from_numpy(rng.standard_normal(n).astype(F32)).to(DEV) if has else None
    a = torch.from_numpy(rng.standard_normal(n).astype(F32)).to(DEV) if has else None
    with np.errstate(invalid="ignore"):
        t = O.dgc_memory_compensate(gw, _np(r) if has else None, _np(a) if has else None, MOM)[0]
    order = np.argsort(np.where(np.isfinite(t), np.abs(t), 0), kind="stable")
    # every sample the largest finite |t| (a handful selected: the loop runs), or the 400th largest
    # (the target count exactly: thr0 stands)
    sidx = np.full(ns_of(n), order[-1] if sample == "largest" else order[-int(n * RATIO)], dtype=np.int64)
    sd = torch.from_numpy(sidx).to(DEV)
    e = _oracle_step(gw, _np(r) if has else None, _np(a) if has else None, sidx)
    assert bool(e["path"]) == (sample == "largest")
    for g_off, st_off in ((0, 0), (1, 0), (2, 0), (4, 0), (0, 1), (0, 2), (4, 2), (1, 1)):
        out, ro, ao = _raw_fused(gb, r, a, has, sd, g_off, st_off)
        what = (has, sample, g_off, st_off)
        assert int(_meta()[4]) == (1 if e["path"] else 0), what
        assert np.array_equal(_out_bits(out), _want_bits(e["out"])), what
        assert same_bits(_np(ro), e["r"]) and same_bits(_np(ao), e["a"]), what


@pytest.mark.parametrize("name", sorted(LOOP_CASES))
def test_threshold_loop_cases_rounded_to_bf16(name):
    """tests/dgc_edge_util.LOOP_CASES with x rounded to bf16, through the fused step: meta.fix says
    whether the speculative result stood (the oracle's path is empty) or the gated fix-up produced
    the output."""
    case = rounded_case(name)
    if name in LOOP_PATH_HOLDS:
        case.check_path()
    n = case.x.size
    gb, gw = bf16_pair(case.x)
    assert same_bits(gw, case.x)
    e = _oracle_step(case.x, None, None, case.sidx, case.ratio)
    out, rn, an = ops.dgc_step_w1_fused(gb.to(DEV), None, None, False, MOM, case.ratio,
                                        sample_idx=torch.from_numpy(case.sidx).to(DEV))
    assert int(_meta()[4]) == (1 if e["path"] else 0), (name, e["path"])
    _check_meta(e, name)
    assert out.dtype == BF16 and out.numel() == n
    assert np.array_equal(_out_bits(out), _want_bits(e["out"])), name
    assert same_bits(_np(rn), e["r"]) and same_bits(_np(an), e["a"]), name


def test_bf16_step_equals_the_f32_step_rounded():
    n = 49154
    rb = ab = rf = af = None
    for s in range(STEPS):
        gb, _ = _grad(n, 300 + s)
        sd = torch.from_numpy(np.random.default_rng(s).integers(0, n, ns_of(n))).to(DEV)
        ob, rb, ab = ops.dgc_step_w1_fused(gb, rb, ab, s > 0, MOM, RATIO, sample_idx=sd)
        of, rf, af = ops.dgc_step_w1_fused(gb.float(), rf, af, s > 0, MOM, RATIO, sample_idx=sd)
        assert np.array_equal(_out_bits(ob), _want_bits(_np(of))), s
        assert same_bits(_np(rb), _np(rf)) and same_bits(_np(ab), _np(af)), s


@pytest.mark.parametrize("clipping", [False, True])
def test_one_name_stepped_bf16_f32_bf16_shares_its_state(clipping):
    ours, parent = _classes()
    n = 40000
    comm, ref = _comm(ours, clipping), _comm(parent, clipping)
    for s, dtype in enumerate((BF16, torch.float32, BF16)):
        gb, _ = _grad(n, 400 + s, specials=False)
        torch.manual_seed(60 + s)
        out = comm.step(gb.to(dtype), "w")
        torch.manual_seed(60 + s)
        want = ref.step(gb.float(), "w")
        assert out.dtype == dtype, s
        if dtype == BF16:
            assert np.array_equal(_out_bits(out), _want_bits(_np(want))), s
        else:
            assert same_bits(_np(out), _np(want)), s
        assert same_bits(_np(comm.memory.residuals["w"]), _np(ref.memory.residuals["w"])), s
        assert same_bits(_np(comm.memory.gradients["w"]), _np(ref.memory.gradients["w"])), s


# ------------------------------------------------------------------------------- pieces
@pytest.mark.parametrize("n", [7, 40003])
@pytest.mark.parametrize("has", [False, True])
def test_sample_comp_and_compensate_equal_the_f32_forms(n, has):
    gb, gw = _grad(n, 500 + n)
    rng = np.random.default_rng(n)
    r0, a0 = rng.standard_normal(n).astype(F32), rng.standard_normal(n).astype(F32)
    sd = torch.from_numpy(rng.integers(0, n, 64)).to(DEV)

    def state():
        return torch.from_numpy(r0.copy()).to(DEV), torch.from_numpy(a0.copy()).to(DEV)
    r, a = state()
    got = ops.dgc_sample_comp(gb, r, a, has, MOM, 64, sample_idx=sd)
    want = ops.dgc_sample_comp(gb.float(), r, a, has, MOM, 64, sample_idx=sd)
    assert same_bits(_np(got), _np(want))
    t, er, ea = O.dgc_memory_compensate(gw, r0 if has else None, a0 if has else None, MOM)
    for off in (0, 1, 2, 4):
        buf = torch.empty(n + 8, dtype=BF16, device=DEV)
        g = buf[off:off + n].copy_(gb)
        r, a = state()
        ops.dgc_compensate(g, r, a, has, MOM)
        assert same_bits(_np(r), er) and same_bits(_np(a), ea), (n, has, off)


# ------------------------------------------------------------------------------- clipping
def _root_far_from_tie(x):
    """Whether sqrt(x), x an f32 value given as a double, is at least 0.01 ulp from the midpoint of
    its two f32 neighbours (the root in double is good to 1e-9 ulp of f32)."""
    root = float(np.sqrt(np.float64(x)))
    lo = np.float32(root)
    if float(lo) > root:
        lo = np.nextafter(lo, F32(0))
    ulp = float(np.nextafter(lo, F32(np.inf))) - float(lo)
    return abs((root - float(lo)) / ulp - 0.5) >= 0.01


@pytest.mark.parametrize("n", [7, 16389, 300001])      # 300001: more than one trip of sumsq's 1024-workgroup grid
def test_sumsq_and_clip_equal_the_f32_forms_and_the_oracle(n):
    # The oracle takes its bound from the host's f32 sqrt, which is not correctly rounded on every host
    # when the exact root lies within a thousandth of an ulp of a rounding tie (seen: sqrt(5.3661385 / 2),
    # 0.0006 ulp above the tie, rounded down).  The kernel's sqrt is correctly rounded; so the first seed
    # whose two bounds are a hundredth of an ulp or more from a tie is taken, by this test of s alone.
    for seed in range(600 + n, 620 + n):
        gb, gw = _grad(n, seed, specials=False)
        s = ops.sumsq(gb)
        assert s.dtype == torch.float32 and same_bits(_np(s), _np(ops.sumsq(gb.float())))
        if all(_root_far_from_tie(float(_np(s)[0]) / world) for world in (1, 2)):
            break
    else:
        raise AssertionError("no seed with both bounds away from a rounding tie")
    for world in (1, 2):
        got = ops.clip_by_sumsq(gb, s, world)
        assert got.dtype == torch.float32
        assert same_bits(_np(got), O.dgc_clip(gw, _np(s), world)), (n, world)
    gb, gw = _grad(n, 601 + n, specials=True)           # a NaN in g makes the bound NaN: every element NaN
    s = ops.sumsq(gb)
    assert same_bits(_np(s), _np(ops.sumsq(gb.float())))
    assert same_bits(_np(ops.clip_by_sumsq(gb, s, 1)), _np(ops.clip_by_sumsq(gb.float(), s, 1)))


@pytest.mark.parametrize("n", [7, 16389, 40000])
def test_clipping_step_vs_oracle(n):
    """gradient_clipping=True at world 1: bf16 sumsq, clip to f32, f32 compensate, select, and the
    mask pass that writes bf16 (grace_dgc_step_w1_bf16)."""
    comm = _comm(_classes()[0], clipping=True)
    r = a = None
    for s in range(STEPS):
        gb, gw = _grad(n, 700 + 10 * n + s, specials=False)
        ssq = _np(ops.sumsq(gb))
        clipped = O.dgc_clip(gw, ssq, 1)
        sidx = _draw(n, 70 + s)
        e = _oracle_step(clipped, r, a, sidx)
        torch.manual_seed(70 + s)
        out = comm.step(gb, "w")
        assert np.array_equal(_out_bits(out), _want_bits(e["out"])), (n, s)
        assert same_bits(_np(comm.memory.residuals["w"]), e["r"]), (n, s)
        assert same_bits(_np(comm.memory.gradients["w"]), e["a"]), (n, s)
        _check_meta(e, (n, s), slot="dgc")
        r, a = e["r"], e["a"]


def test_step_w1_bf16_misaligned_out():
    n = 40003
    rng = np.random.default_rng(9)
    t0, r0 = rng.standard_normal(n).astype(F32), rng.standard_normal(n).astype(F32)
    t0[:4] = [np.nan, np.inf, -np.inf, -0.0]
    sd = torch.from_numpy(rng.integers(4, n, ns_of(n))).to(DEV)
    want = None
    for off in (0, 1, 2, 4):
        t, r = torch.from_numpy(t0.copy()).to(DEV), torch.from_numpy(r0.copy()).to(DEV)
        ws = ops.dgc_select(t, RATIO, sample_idx=sd)
        out = torch.empty(n + 8, dtype=BF16, device=DEV)[off:off + n]
        got = ops.dgc_step_w1(t, r, t, ws, out=out, out_dtype=BF16)
        assert got.data_ptr() == out.data_ptr()
        t2, r2 = torch.from_numpy(t0.copy()).to(DEV), torch.from_numpy(r0.copy()).to(DEV)
        want = ops.dgc_step_w1(t2, r2, t2, ops.dgc_select(t2, RATIO, sample_idx=sd))
        assert np.array_equal(_out_bits(got), _want_bits(_np(want))), off
        assert same_bits(_np(r), _np(r2)) and same_bits(_np(t), _np(t2)), off
    assert np.count_nonzero(_np(want)) > 0


# ------------------------------------------------------------------------------- dtypes, call order
def test_float16_raises_typeerror():
    comm = _comm(_classes()[0])
    with pytest.raises(TypeError):
        comm.step(torch.zeros(256, dtype=torch.float16, device=DEV), "w")
    with pytest.raises(TypeError):
        ops.dgc_step_w1_fused(torch.zeros(256, dtype=torch.float16, device=DEV), None, None, False, MOM, RATIO)


@pytest.fixture
def trace(monkeypatch):
    """trace(run) -> the names run() hands to _lib.call, on its second execution."""
    names = []
    real = _lib.call

    def recording(name, *args):
        names.append(name)
        return real(name, *args)
    monkeypatch.setattr(_lib, "call", recording)

    def trace(run):
        run()
        del names[:]
        run()
        return list(names)
    return trace


SAMPLE = ["grace_dgc_sample_kth"]
BF16_CALLS = {
    False: (["grace_dgc_sample_comp_bf16"] + SAMPLE + ["grace_dgc_step_w1_fused_bf16"]) * STEPS,
    True: (["grace_sumsq_bf16", "grace_clip_by_sumsq_bf16", "grace_dgc_compensate", "grace_dgc_sample"] + SAMPLE
           + ["grace_dgc_select", "grace_dgc_step_w1_bf16"]) * STEPS,
}


@pytest.mark.parametrize("clipping", [False, True])
def test_call_order(trace, clipping):
    """A float32 gradient through the new class makes the parent's native calls in the parent's
    order; a bfloat16 one makes the sequence written here."""
    ours, parent = _classes()

    def steps(cls, dtype):
        def run():
            comm = _comm(cls, clipping)
            for s in range(STEPS):
                torch.manual_seed(80 + s)
                comm.step(_grad(16389, 800 + s, specials=False)[0].to(dtype), "w")
            torch.cuda.synchronize()
        return run
    want = trace(steps(parent, torch.float32))
    got = trace(steps(ours, torch.float32))
    assert want and got == want
    got = trace(steps(ours, BF16))
    print("bf16", clipping, got)
    assert got == BF16_CALLS[clipping]
