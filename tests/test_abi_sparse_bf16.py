"""The entry points of include/grace_hip_sparse.h are declared, exported and bound in
_lib.SIGNATURES_SPARSE, the twin mirrors its f32 form, bad arguments are refused without touching the
device, and the first four headers and tables are what they were.  The dtype checks of the ops
wrappers, the class relations of grace_amd.sparse_bf16, the two bodies it repeats from its parent and
what the GPU tests lean on (the overflowing world-2 gradients, the numpy reference of the padded
decode) need no GPU either."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

from oracle import grace_oracle as O
from tests.abi_util import ROOT, OnGpu, body, check_bad, check_types, declared, header, no_native, params
from tests.golden_util import same_bits
from tests.sparse_bf16_util import padded_ref

F32 = np.float32
NEW = ("grace_axpby_bf16", "grace_randomk_aggregate_bf16", "grace_randomk_clear", "grace_randomk_step_w1_dense_bf16",
       "grace_sparse_aggregate_padded_bf16", "grace_sparse_aggregate_padded_bf16_workspace_bytes",
       "grace_threshold_step_w1_bf16")


def test_entry_points_declared_exported_bound():
    from grace_amd import _lib
    hdr = header("grace_hip_sparse.h")
    assert '#include "grace_hip.h"' in hdr and 'extern "C"' in hdr
    assert declared(hdr) == sorted(NEW) == sorted(_lib.SIGNATURES_SPARSE)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert hasattr(lib, name), f"{name} is not exported by the library"
    bound = _lib.load()
    for name, (res, args) in _lib.SIGNATURES_SPARSE.items():
        f = getattr(bound, name)
        assert f.restype == res and list(f.argtypes) == args, name
        assert res is (_lib.SZ if name.endswith("_bytes") else _lib.ST)
    check_types(hdr, _lib.SIGNATURES_SPARSE)      # each bound type is the prototype's
    raw = open(os.path.join(ROOT, "include", "grace_hip_sparse.h")).read()
    for name in NEW:   # a doc comment right above every entry point
        assert re.search(r"\*/\s*\n[a-z_ ]+\b%s\(" % name, raw), f"{name} has no doc comment"


def test_first_four_headers_and_tables_are_unchanged():
    from grace_amd import _lib
    for h, table, count in (("grace_hip.h", _lib.SIGNATURES, 159), ("grace_hip_sign.h", _lib.SIGNATURES_SIGN, 11),
                            ("grace_hip_quant.h", _lib.SIGNATURES_QUANT, 6),
                            ("grace_hip_dgc.h", _lib.SIGNATURES_DGC, 8)):
        names = declared(header(h))
        assert len(names) == count and len(table) == count and sorted(table) == names, h
        assert not set(NEW) & set(names)


def test_threshold_twin_mirrors_the_f32_entry_point():
    from grace_amd import _lib
    want = params(header("grace_hip.h"), "grace_threshold_step_w1")
    for s in ("const float* g", "float* out"):
        assert want.count(s) == 1, s
        want = want.replace(s, s.replace("float*", "uint16_t*"))
    assert params(header("grace_hip_sparse.h"), "grace_threshold_step_w1_bf16") == want
    assert _lib.SIGNATURES_SPARSE["grace_threshold_step_w1_bf16"] == _lib.SIGNATURES["grace_threshold_step_w1"]
    # the dense random-k twin drops the recycled output's two grouping buffers and nothing else
    f32 = params(header("grace_hip.h"), "grace_randomk_step_w1_dense")
    for s in ("const float* g", "float* out"):
        f32 = f32.replace(s, s.replace("float*", "uint16_t*"))
    f32 = f32.replace(" void* grp, const void* prev_grp,", "")
    assert params(header("grace_hip_sparse.h"), "grace_randomk_step_w1_dense_bf16") == f32


def test_argument_errors_do_not_touch_the_device():
    """A null required pointer, a negative size and the stated limits return -1 with "name: ..."; an
    empty input is GRACE_OK where stated.  The pointers are host addresses: a launch would fault."""
    from grace_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_uint64 * 64)()
    p = ctypes.addressof(buf)
    q, r, s = p + 64, p + 128, p + 192

    # g, residual, mode, beta, gamma, n, thr, ws, out, stream
    good = [p, q, 2, 0.9, 0.7, 16, 1.5, r, s, None]
    check_bad(lib, "grace_threshold_step_w1_bf16", good,
              [(0, None), (1, None), (7, None), (8, None), (2, -1), (2, 3), (5, 0), (5, -1)])

    # r, g, has_residual, beta, gamma, t, n, stream
    good = [p, q, 1, 0.9, 0.7, r, 16, None]
    check_bad(lib, "grace_axpby_bf16", good, [(0, None), (1, None), (5, None), (6, -1)])
    good[6] = 0
    assert lib.grace_axpby_bf16(*good) == 0

    # g, residual, has_residual, beta, gamma, n, idx, k, out, ws, ws_bytes, stream
    need = lib.grace_randomk_step_w1_dense_workspace_bytes(16, 4)
    good = [p, q, 1, 0.9, 0.7, 16, r, 4, s, p, need, None]
    check_bad(lib, "grace_randomk_step_w1_dense_bf16", good,
              [(0, None), (1, None), (6, None), (8, None), (9, None), (5, 0), (5, -1), (5, (1 << 28) + 1), (7, -1),
               (10, need - 1)])

    # idx, vals, k, r, n, stream
    good = [p, q, 4, r, 16, None]
    check_bad(lib, "grace_randomk_clear", good, [(0, None), (1, None), (3, None), (2, -1), (4, 0)])
    good[2] = 0
    assert lib.grace_randomk_clear(*good) == 0

    # vals, idx, k, world, divisor, out, n, stream
    good = [p, q, 4, 2, 2.0, r, 16, None]
    check_bad(lib, "grace_randomk_aggregate_bf16", good,
              [(0, None), (1, None), (5, None), (2, -1), (3, 0), (3, -1), (6, 0), (6, -1)])

    # base, cap, counts, world, divisor, out, n, ws, ws_bytes, stream
    wsb = lib.grace_sparse_aggregate_padded_bf16_workspace_bytes
    assert wsb(2, 100) >= 4 * 2 * 2 and wsb(8, 1 << 26) >= 4 * 8 * 8193
    assert wsb(0, 100) == wsb(1025, 100) == wsb(2, 0) == wsb(2, 1 << 31) == 0
    good = [p, 8, q, 2, 2.0, r, 100, s, wsb(2, 100), None]
    bad = [(0, None), (2, None), (5, None), (7, None), (1, 0), (1, -1), (1, 101), (3, 0), (3, -1), (3, 1025), (6, 0),
           (6, 7), (6, 1 << 31), (8, 0), (8, wsb(2, 100) - 1)]
    check_bad(lib, "grace_sparse_aggregate_padded_bf16", good, bad)


def test_ops_check_dtypes_and_limits_before_any_native_call(monkeypatch):
    from grace_amd import ops
    no_native(monkeypatch)
    f32 = torch.zeros(256).as_subclass(OnGpu)
    bf = torch.zeros(256, dtype=torch.bfloat16).as_subclass(OnGpu)
    idx = torch.zeros(4, dtype=torch.int64).as_subclass(OnGpu)
    for dtype in (torch.float16, torch.float64, torch.int16):
        x = torch.zeros(256, dtype=dtype).as_subclass(OnGpu)
        for call in (lambda: ops.threshold_step_w1(x, None, 0, 1.0, 1.0, 1.5), lambda: ops.axpby_grad(None, x, 1.0, 1.0),
                     lambda: ops.randomk_step_w1_dense_bf16(x, f32, False, 1.0, 1.0, idx)):
            with pytest.raises(TypeError) as e:
                call()
            assert not isinstance(e.value, ops.GraceDeviceError), dtype
        with pytest.raises(TypeError):
            ops.randomk_aggregate(f32, idx, 2, 100, 2, out_dtype=dtype)
        with pytest.raises(TypeError):
            ops.sparse_aggregate_padded(f32, 8, idx.to(torch.int32), 2, 100, 2, out_dtype=dtype)
    for x in (torch.zeros(256), torch.zeros(256, dtype=torch.bfloat16)):      # not on the GPU: the device check
        for call in (lambda: ops.threshold_step_w1(x, None, 0, 1.0, 1.0, 1.5), lambda: ops.axpby_grad(None, x, 1.0, 1.0)):
            with pytest.raises(ops.GraceDeviceError):
                call()
    # the residual of a bf16 step is the f32 class's: bf16, short or strided is a TypeError
    for bad in (bf, torch.zeros(255).as_subclass(OnGpu), torch.zeros(512)[::2].as_subclass(OnGpu), None):
        for call in (lambda: ops.threshold_step_w1(bf, bad, 2, 0.9, 0.7, 1.5),
                     lambda: ops.randomk_step_w1_dense_bf16(bf, bad, True, 0.9, 0.7, idx)):
            with pytest.raises(TypeError):
                call()
        if bad is not None:
            with pytest.raises(TypeError):
                ops.axpby_grad(bad, bf, 0.9, 0.7)
    with pytest.raises(TypeError):
        ops.randomk_step_w1_dense_bf16(f32, f32, False, 1.0, 1.0, idx)           # f32 has its own entry
    cnt = torch.zeros(2, dtype=torch.int32).as_subclass(OnGpu)
    for cap, world, n in ((8, 2, 7), (0, 2, 100), (8, 2, 1 << 31), (1, 1025, 100)):
        with pytest.raises(ValueError):
            ops.sparse_aggregate_padded(torch.zeros(1025 * 16).as_subclass(OnGpu), cap, cnt, world, n, 1)


def test_classes_are_the_dist_classes():
    from grace_amd import sparse_bf16 as S
    from grace_amd.dist.compressor.randomk import RandomKCompressor
    from grace_amd.dist.compressor.threshold import ThresholdCompressor
    assert issubclass(S.ThresholdCompressor, ThresholdCompressor) and S.ThresholdCompressor is not ThresholdCompressor
    assert issubclass(S.RandomKCompressor, RandomKCompressor) and S.RandomKCompressor is not RandomKCompressor
    for attr in ("compress", "decompress", "decode_aggregate_variable", "_grow", "_settle", "_counts_exchange",
                 "__init__"):
        assert getattr(S.ThresholdCompressor, attr) is getattr(ThresholdCompressor, attr), attr
    for attr in ("compress", "decompress", "_indices", "__init__"):
        assert getattr(S.RandomKCompressor, attr) is getattr(RandomKCompressor, attr), attr
    c = S.ThresholdCompressor(0.5, exchange="capacity", capacity_margin=1.5, overflow="defer")
    assert (c.threshold, c.exchange, c.capacity_margin, c.overflow, c.tensors_size_are_same) == (0.5, "capacity", 1.5,
                                                                                                 "defer", False)
    with pytest.raises(ValueError):
        S.ThresholdCompressor(0.5, exchange="sizes")
    k = S.RandomKCompressor(0.25, rng="torch_cpu", recycle_output=False)
    assert (k.compress_ratio, k.rng, k.recycle_output, k.global_step) == (0.25, "torch_cpu", False, 0)


def test_counts_exchange_is_the_parents_but_for_the_decode():
    """grace_amd/dist/ has no hook at the decode, so the stand-in repeats _counts_exchange: its body is
    the parent's text with the two f32 decode calls replaced by the padded bf16 decode, nothing else."""
    from grace_amd import sparse_bf16 as S
    from grace_amd.dist.compressor.threshold import ThresholdCompressor
    parent, ours = body(ThresholdCompressor._counts_exchange), body(S.ThresholdCompressor._counts_exchange_bf16)
    at = [i for i, ln in enumerate(parent) if "ops.sparse_aggregate(" in ln]
    assert len(at) == 2 and parent[at[0] + 1].strip() == "W if self.average else 1)"
    want = list(parent)
    want[at[1]] = "        out = ops.sparse_aggregate_padded(send, cap, counts_dev, 1, n, 1)"
    want[at[0]:at[0] + 2] = ["        out = ops.sparse_aggregate_padded(recv, cap, counts_dev, W, n, "
                             "W if self.average else 1)"]
    assert ours == want
    assert list(inspect.signature(S.ThresholdCompressor._counts_exchange_bf16).parameters) == \
        list(inspect.signature(ThresholdCompressor._counts_exchange).parameters)


def test_exchange_step_is_the_parents_fused_step_from_its_count_on():
    """... and _exchange_step is the parent's fused_step from the workspace line of its exchange part to
    its end, with the counts exchange renamed and `out_dtype=BF16` added to the records decode."""
    from grace_amd import sparse_bf16 as S
    from grace_amd.dist.compressor.threshold import ThresholdCompressor
    parent, ours = body(ThresholdCompressor.fused_step), body(S.ThresholdCompressor._exchange_step)
    starts = [i for i, ln in enumerate(parent) if ln.strip().startswith('ws = ops.workspace("threshold"')]
    assert len(starts) == 2                                   # the world-1 fused pass, then the exchange part
    tail = parent[starts[1]:]
    assert sum("self._counts_exchange(" in ln for ln in tail) == 2
    assert sum("ops.sparse_aggregate_capped(" in ln for ln in tail) == 1
    want = [ln.replace("self._counts_exchange(", "self._counts_exchange_bf16(")
            .replace(", stat)", ", stat, out_dtype=BF16)") if "ops.sparse_aggregate_capped(" in ln
            else ln.replace("self._counts_exchange(", "self._counts_exchange_bf16(") for ln in tail]
    head = ["    n = t.numel()", "    dev = t.device", "    residual = type(mem) is ResidualMemory"]
    assert ours == head + want


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_by_hand_still_refuses(dtype):
    """compress and the memories are the parents': bf16 and float16 raise TypeError by hand, and so does
    the Allgather step on a tensor that is not on the GPU; random-k with NoneMemory fuses nothing."""
    from grace_amd import sparse_bf16 as S
    from grace_amd.dist.communicator.allgather import Allgather
    from grace_amd.dist.memory.none import NoneMemory
    from grace_amd.dist.memory.residual import ResidualMemory
    x = torch.zeros(256, dtype=dtype)
    for comp in (S.ThresholdCompressor(1.5), S.RandomKCompressor(0.5)):
        for t in (x, x.as_subclass(OnGpu)):
            with pytest.raises(TypeError):
                comp.compress(t, "w")
        for mem in (NoneMemory(), ResidualMemory()):
            with pytest.raises(TypeError):
                Allgather(comp, mem, 1).step(x, "w")
    with pytest.raises(TypeError):
        Allgather(S.RandomKCompressor(0.5), NoneMemory(), 1).step(x.as_subclass(OnGpu), "w")


def test_limits_raise_value_error_before_anything_runs(monkeypatch):
    from grace_amd import sparse_bf16 as S
    from grace_amd.dist.communicator.allgather import Allgather
    from grace_amd.dist.memory.residual import ResidualMemory
    no_native(monkeypatch)

    class Big(OnGpu):
        size = 1 << 31

        def numel(self):
            return self.size
    x = torch.zeros(4, dtype=torch.bfloat16).as_subclass(Big)
    comm = Allgather(S.ThresholdCompressor(1.5), ResidualMemory(), 2)
    with pytest.raises(ValueError, match="2\\^31"):
        comm.compressor.fused_step(comm, x, "w")
    Big.size = (1 << 28) + 1
    comm = Allgather(S.RandomKCompressor(0.01), ResidualMemory(), 1)
    with pytest.raises(ValueError, match="2\\^28"):
        comm.compressor.fused_step(comm, x, "w")
    assert comm.compressor.global_step == 0          # refused before the draw


# ------------------------------------------------------------------ what the GPU tests lean on
def test_world2_margin_one_runs_still_overflow_at_step_2_on_rounded_gradients():
    """tests/test_gpu_sparse_bf16_world2.py asserts `overflows >= 1` for its margin-1.0 runs: with the
    gradients rounded to bf16 the 3x tail of rank 1 at step 2 still selects more than the capacity the
    steps before it set."""
    from tests.sparse_bf16_util import world2_thr_grad
    from tests.test_gpu_sparse_bf16_world2 import THR_RUNS, expected_threshold
    seen = 0
    for key, exchange, margin, overflow, memory, _ in THR_RUNS:
        if exchange != "capacity":
            continue
        assert margin == 1.0
        _, overflows, over_steps = expected_threshold(exchange, margin, overflow, memory)
        assert overflows >= 1 and 2 in over_steps, (key, overflows, over_steps)
        seen += 1
    assert seen == 3
    g = world2_thr_grad("cap", 1, 2)
    assert np.array_equal(g.view(np.uint32) & 0xFFFF, np.zeros(g.size, dtype=np.uint32))


def test_padded_reference_agrees_with_the_oracle():
    """padded_ref restates O.sparse_decode per rank + O.python_sum + the division on a small case (with
    -0, a shared index, a zero count and garbage past the counts)."""
    n, cap = 37, 6
    rng = np.random.default_rng(3)
    counts = np.array([6, 0, 4], dtype=np.int32)
    vals = rng.standard_normal((3, cap)).astype(F32)
    idx = np.sort(np.stack([rng.choice(n, cap, replace=False) for _ in range(3)]), axis=1).astype(np.int32)
    idx[2, 0], vals[2, 0], vals[0, 1] = idx[0, 0], F32(-0.0), F32(-0.0)      # a shared index; -0 + -0 after the 0
    idx[2, 4:], vals[2, 4:] = 2 ** 31 - 1, F32(1e30)                          # garbage past the count
    assert (np.diff(idx[2, :4]) > 0).all()
    decs = [O.sparse_decode(vals[w][:counts[w]], idx[w][:counts[w]], n) for w in range(3)]
    for divisor in (3, 1):
        want = (O.python_sum(decs) / F32(divisor)).astype(F32)
        assert same_bits(padded_ref(vals, idx, counts, cap, n, divisor), want)
