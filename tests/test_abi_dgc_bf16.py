"""The entry points of include/grace_hip_dgc.h are declared, exported and bound in
_lib.SIGNATURES_DGC, the twins mirror their f32 forms, bad arguments are refused without touching the
device, and the first three headers and tables are what they were.  The dtype checks of the ops
wrappers, the class relations of grace_amd.dgc_bf16, the one method it repeats from its parent and
the inputs the GPU tests lean on (the threshold-loop cases rounded to bf16, the overflowing world-2
gradients) need no GPU either."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

from tests.abi_util import ROOT, OnGpu, body, check_bad, declared, header, no_native, params
from tests.dgc_bf16_util import LOOP_PATH_HOLDS, LOOP_PATH_LOST, rounded_case, world2_grad
from tests.dgc_edge_util import LOOP_CASES

# f32 form -> its parameters that become uint16_t* in the twin
TWINS = {
    "grace_dgc_step_w1_fused": ("const float* g", "float* out"),
    "grace_dgc_sample_comp": ("const float* g",),
    "grace_dgc_compensate": ("const float* g",),
    "grace_dgc_step_w1": ("float* out",),
    "grace_sumsq": ("const float* x",),
    "grace_clip_by_sumsq": ("const float* x",),
}
DECODE = ("grace_sparse_aggregate_records_bf16", "grace_sparse_aggregate_records_bf16_workspace_bytes")
NEW = tuple(sorted([f + "_bf16" for f in TWINS] + list(DECODE)))


def test_entry_points_declared_exported_bound():
    from grace_amd import _lib
    dgc = header("grace_hip_dgc.h")
    assert '#include "grace_hip.h"' in dgc and 'extern "C"' in dgc
    assert declared(dgc) == sorted(NEW) == sorted(_lib.SIGNATURES_DGC)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert hasattr(lib, name), f"{name} is not exported by the library"
    bound = _lib.load()
    for name, (res, args) in _lib.SIGNATURES_DGC.items():
        f = getattr(bound, name)
        assert f.restype == res and list(f.argtypes) == args, name
        assert len(args) == params(dgc, name).count(",") + 1, name
    raw = open(os.path.join(ROOT, "include", "grace_hip_dgc.h")).read()
    for name in NEW:   # a doc comment right above every entry point
        assert re.search(r"\*/\s*\n[a-z_ ]+\b%s\(" % name, raw), f"{name} has no doc comment"


def test_first_three_headers_and_tables_are_unchanged():
    from grace_amd import _lib
    for h, table, count in (("grace_hip.h", _lib.SIGNATURES, 159), ("grace_hip_sign.h", _lib.SIGNATURES_SIGN, 11),
                            ("grace_hip_quant.h", _lib.SIGNATURES_QUANT, 6)):
        names = declared(header(h))
        assert len(names) == count and len(table) == count and sorted(table) == names, h
        assert not set(NEW) & set(names)


@pytest.mark.parametrize("f32", sorted(TWINS))
def test_bf16_twin_mirrors_the_f32_entry_point(f32):
    from grace_amd import _lib
    want = params(header("grace_hip.h"), f32)
    for s in TWINS[f32]:
        assert want.count(s) == 1, (f32, s)
        want = want.replace(s, s.replace("float*", "uint16_t*"))
    assert params(header("grace_hip_dgc.h"), f32 + "_bf16") == want
    assert _lib.SIGNATURES_DGC[f32 + "_bf16"] == _lib.SIGNATURES[f32]


def test_argument_errors_do_not_touch_the_device():
    """A null required pointer, a negative size, new state aliasing the old and the decode's limits
    return -1 with "name: ..."; an empty input is GRACE_OK where the f32 form has that rule.  The
    pointers are host addresses: a launch would fault."""
    from grace_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_uint64 * 64)()
    p = ctypes.addressof(buf)
    q, r, s = p + 64, p + 128, p + 192

    # g, residual, accum, has_state, momentum, n, top_vals, ks, ratio, ws, residual_out, accum_out, out, stream
    name = "grace_dgc_step_w1_fused_bf16"
    good = [p, q, r, 1, 0.9, 16, p, 1, 0.01, p, s, s + 64, p, None]
    bad = [(0, None), (1, None), (2, None), (6, None), (9, None), (10, None), (11, None), (12, None), (5, 0), (5, -1),
           (5, 1 << 40), (7, 0), (10, q), (11, r), (11, s)]
    check_bad(lib, name, good, bad)

    # g, residual, accum, has_state, momentum, n, sample_idx, seed, ns, sample_abs, stream
    name = "grace_dgc_sample_comp_bf16"
    good = [p, q, r, 1, 0.9, 16, None, 1, 4, s, None]
    check_bad(lib, name, good, [(0, None), (1, None), (2, None), (9, None), (5, 0), (5, -1), (8, 0), (8, -1)])

    # g, residual, accum, has_state, momentum, n, stream
    name = "grace_dgc_compensate_bf16"
    good = [p, q, r, 1, 0.9, 16, None]
    check_bad(lib, name, good, [(0, None), (1, None), (2, None), (5, -1), (2, q)])
    good[5] = 0
    assert getattr(lib, name)(*good) == 0

    # t, residual, accum, n, ws, out, stream
    name = "grace_dgc_step_w1_bf16"
    good = [p, q, r, 16, p, s, None]
    check_bad(lib, name, good, [(0, None), (1, None), (2, None), (4, None), (5, None), (3, -1), (2, q)])
    good[3] = 0
    assert getattr(lib, name)(*good) == 0

    # x, n, ws, out, stream
    check_bad(lib, "grace_sumsq_bf16", [p, 16, q, r, None], [(0, None), (2, None), (3, None), (1, -1)])
    # x, sumsq_dev, world, out, n, stream
    name = "grace_clip_by_sumsq_bf16"
    good = [p, q, 2.0, r, 16, None]
    check_bad(lib, name, good, [(0, None), (1, None), (3, None), (4, -1), (2, 0.0), (2, -1.0)])
    good[4] = 0
    assert getattr(lib, name)(*good) == 0

    # recs, stride, cap, world, divisor, out, n, stat, ws, ws_bytes, stream
    name = "grace_sparse_aggregate_records_bf16"
    wsb = lib.grace_sparse_aggregate_records_bf16_workspace_bytes
    assert wsb(2, 100) >= 4 * 2 * 2 and wsb(8, 1 << 26) >= 4 * 8 * 8193
    assert wsb(0, 100) == wsb(1025, 100) == wsb(2, 0) == wsb(2, 1 << 31) == 0
    good = [p, 4 + 2 * 8, 8, 2, 2.0, q, 100, r, s, wsb(2, 100), None]
    bad = [(0, None), (5, None), (7, None), (8, None), (1, 4 + 2 * 8 + 1), (2, 0), (2, -1), (2, 101), (3, 0), (3, -1),
           (3, 1025), (6, 0), (6, 7), (6, 1 << 31), (9, 0), (9, wsb(2, 100) - 1)]
    check_bad(lib, name, good, bad)


def test_ops_check_dtypes_before_any_native_call(monkeypatch):
    from grace_amd import ops
    no_native(monkeypatch)
    f32 = torch.zeros(256)
    for dtype in (torch.float16, torch.float64, torch.int16):
        for x in (torch.zeros(256, dtype=dtype), torch.zeros(256, dtype=dtype).as_subclass(OnGpu)):
            for call in (lambda: ops.dgc_sample_comp(x, None, None, False, 0.9, 2),
                         lambda: ops.dgc_compensate(x, f32, f32.clone(), False, 0.9),
                         lambda: ops.dgc_step_w1_fused(x, None, None, False, 0.9, 0.01),
                         lambda: ops.sumsq(x), lambda: ops.clip_by_sumsq(x, f32[:1], 1)):
                with pytest.raises(TypeError) as e:
                    call()
                if isinstance(x, OnGpu):   # on the device it is the dtype that is refused
                    assert not isinstance(e.value, ops.GraceDeviceError), dtype
        with pytest.raises(TypeError):
            ops.dgc_step_w1(f32, f32, f32, None, out_dtype=dtype)
        with pytest.raises(TypeError):
            ops.sparse_aggregate_capped(torch.zeros(20, dtype=torch.int32), 8, 1, 100, 1, f32, out_dtype=dtype)
    for dtype in (torch.float32, torch.bfloat16):   # accepted dtypes on the CPU: the device check, no native call
        x = torch.zeros(256, dtype=dtype)
        for call in (lambda: ops.dgc_sample_comp(x, None, None, False, 0.9, 2),
                     lambda: ops.dgc_compensate(x, f32, f32.clone(), False, 0.9),
                     lambda: ops.dgc_step_w1_fused(x, None, None, False, 0.9, 0.01),
                     lambda: ops.sumsq(x), lambda: ops.clip_by_sumsq(x, f32[:1], 1)):
            with pytest.raises(ops.GraceDeviceError):
                call()


def test_ops_bf16_state_must_be_f32(monkeypatch):
    """The memory of a bf16 step is the f32 class's: a bf16, short or strided residual is a TypeError
    before any native call; the bf16 decode's limits are a ValueError."""
    from grace_amd import ops
    no_native(monkeypatch)
    g = torch.zeros(256, dtype=torch.bfloat16).as_subclass(OnGpu)
    ok = torch.zeros(256).as_subclass(OnGpu)
    for bad in (torch.zeros(256, dtype=torch.bfloat16).as_subclass(OnGpu), torch.zeros(255).as_subclass(OnGpu),
                torch.zeros(512)[::2].as_subclass(OnGpu), None):
        for call in (lambda: ops.dgc_step_w1_fused(g, bad, ok, True, 0.9, 0.01),
                     lambda: ops.dgc_step_w1_fused(g, ok, bad, True, 0.9, 0.01),
                     lambda: ops.dgc_sample_comp(g, bad, ok, True, 0.9, 2),
                     lambda: ops.dgc_compensate(g, bad, ok, False, 0.9),
                     lambda: ops.dgc_compensate(g, ok, bad, True, 0.9)):
            with pytest.raises(TypeError):
                call()
    recs = torch.zeros(2 * 20, dtype=torch.int32).as_subclass(OnGpu)
    monkeypatch.setattr(ops, "exchange_record_words", lambda cap: 4 + 2 * int(cap))
    stat = torch.zeros(2, dtype=torch.int32)
    for cap, world, n in ((8, 2, 7), (8, 2, 1 << 31)):
        with pytest.raises(ValueError):
            ops.sparse_aggregate_capped(recs, cap, world, n, 1, stat, out_dtype=torch.bfloat16)
    with pytest.raises(ValueError):
        ops.sparse_aggregate_capped(torch.zeros(1025 * 6, dtype=torch.int32).as_subclass(OnGpu), 1, 1025, 100, 1, stat,
                                    out_dtype=torch.bfloat16)


def test_class_is_the_dist_class():
    from grace_amd import dgc_bf16 as D
    from grace_amd.dist.compressor.dgc import DgcCompressor
    assert issubclass(D.DgcCompressor, DgcCompressor) and D.DgcCompressor is not DgcCompressor
    for attr in ("compress", "decompress", "_sampling", "_grow", "_settle", "_records", "__init__"):
        assert getattr(D.DgcCompressor, attr) is getattr(DgcCompressor, attr), attr
    assert D.DgcCompressor.fused_step is not DgcCompressor.fused_step
    c = D.DgcCompressor(0.01, rng="torch_cpu", exchange="capacity", capacity_margin=1.5, overflow="defer")
    assert (c.compress_ratio, c.rng, c.exchange, c.capacity_margin, c.overflow) == (0.01, "torch_cpu", "capacity", 1.5,
                                                                                    "defer")
    assert c.tensors_size_are_same is False
    with pytest.raises(ValueError):
        D.DgcCompressor(0.01, exchange="sizes")


def test_exchange_step_is_the_parents_but_for_the_decode_dtype():
    """grace_amd/dist/ has no hook at the decode, so the stand-in repeats _exchange_step: its body is
    the parent's text with `out_dtype=out_dtype` added to the two decode calls, and nothing else."""
    from grace_amd import dgc_bf16 as D
    from grace_amd.dist.compressor.dgc import DgcCompressor
    parent, ours = body(DgcCompressor._exchange_step), body(D.DgcCompressor._exchange_step)
    assert sum("ops.sparse_aggregate_capped(" in ln for ln in parent) == 2
    want = [ln.replace(", stat)", ", stat, out_dtype=out_dtype)") if "ops.sparse_aggregate_capped(" in ln else ln
            for ln in parent]
    assert ours == want
    sig = inspect.signature(D.DgcCompressor._exchange_step)
    assert list(sig.parameters)[:-1] == list(inspect.signature(DgcCompressor._exchange_step).parameters)
    assert sig.parameters["out_dtype"].default is torch.float32


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_by_hand_still_refuses(dtype):
    """compress and DgcMemory.compensate / update are the parents': bf16 and float16 raise TypeError;
    so does the Allgather step on a tensor that is not on the GPU."""
    from grace_amd import dgc_bf16 as D
    from grace_amd.dist.communicator.allgather import Allgather
    from grace_amd.dist.memory.dgc import DgcMemory
    x = torch.zeros(256, dtype=dtype)
    comp = D.DgcCompressor(0.01)
    for t in (x, x.as_subclass(OnGpu)):
        with pytest.raises(TypeError):
            comp.compress(t, "w")
        with pytest.raises(TypeError):
            DgcMemory(0.9, False, 1).compensate(t, "w")
    with pytest.raises(TypeError):
        Allgather(comp, DgcMemory(0.9, False, 1), 1).step(x, "w")


def test_world_above_one_refuses_2p31_elements():
    from grace_amd import dgc_bf16 as D
    from grace_amd.dist.communicator.allgather import Allgather
    from grace_amd.dist.memory.dgc import DgcMemory

    class Big(OnGpu):
        def numel(self):
            return 1 << 31
    comm = Allgather(D.DgcCompressor(0.01), DgcMemory(0.9, False, 2), 2)
    x = torch.zeros(4, dtype=torch.bfloat16).as_subclass(Big)
    with pytest.raises(ValueError, match="2\\^31"):
        comm.compressor.fused_step(comm, x, "w")


# ------------------------------------------------------------------ the inputs the GPU tests lean on
def test_loop_case_lists_cover_every_case():
    assert sorted(LOOP_PATH_HOLDS + LOOP_PATH_LOST) == sorted(LOOP_CASES)
    assert len(LOOP_PATH_HOLDS) == 13 and len(LOOP_PATH_LOST) == 4


@pytest.mark.parametrize("name", LOOP_PATH_HOLDS)
def test_rounded_loop_case_keeps_its_path(name):
    """x rounded to bf16 still drives the oracle's adjustment loop down the path it was built for."""
    case = rounded_case(name)
    assert np.array_equal(case.x.view(np.uint32) & 0xFFFF, np.zeros(case.x.size, dtype=np.uint32))
    case.check_path()


def test_world2_margin_one_runs_still_overflow_on_rounded_gradients():
    """tests/test_gpu_dgc_bf16_world2.py asserts `overflows >= 1` for the margin-1.0 modes: with the
    gradients rounded to bf16 the heavier tail of rank 1 at step 3 still selects more than the
    capacity set by the steps before it."""
    from tests.test_gpu_dgc_bf16_world2 import _expected
    for mode in (("capacity", 1.0, "retry"), ("capacity", 1.0, "defer")):
        _, overflows = _expected(mode)
        assert overflows >= 1, mode
    g = world2_grad(1, 3)
    assert np.array_equal(g.view(np.uint32) & 0xFFFF, np.zeros(g.size, dtype=np.uint32))
