"""grace_shard_select_bf16, grace_shard_clear_bf16 and grace_fill_bf16 are declared, exported and
bound, mirror their f32 twins and refuse bad arguments without touching the device; the checks of
ops.shard_select / ops.shard_clear / ops.fill_bf16 on the output's dtype need no GPU either."""
import ctypes
import re

import pytest
import torch

from tests.abi_util import header, no_native, params

NEW = ("grace_shard_select_bf16", "grace_shard_clear_bf16", "grace_fill_bf16")


def test_entry_points_declared_exported_bound():
    from grace_amd import _lib
    hdr = header("grace_hip.h")
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        params(hdr, name)
        assert hasattr(lib, name), f"{name} is not exported by the library"
        assert name in _lib.SIGNATURES
    assert params(hdr, "grace_fill_bf16") == "uint16_t* x, uint16_t bits, int64_t n, void* stream"
    assert _lib.SIGNATURES["grace_fill_bf16"] == (_lib.ST, [_lib.P, ctypes.c_uint16, _lib.I64, _lib.P])
    # 156 before this change (DESIGN.md §9 "Segmented step"), three more with it
    assert len(set(re.findall(r"\b(grace_[a-z0-9_]+)\s*\(", hdr))) == 159


@pytest.mark.parametrize("f32", ["grace_shard_select", "grace_shard_clear"])
def test_bf16_twin_mirrors_the_f32_entry_point(f32):
    from grace_amd import _lib
    hdr = header("grace_hip.h")
    want = params(hdr, f32)
    assert want.count("float* out") == 1
    assert params(hdr, f32 + "_bf16") == want.replace("float* out", "uint16_t* out")
    assert _lib.SIGNATURES[f32 + "_bf16"] == _lib.SIGNATURES[f32]


def _bad_select_args(p):
    ws = 1 << 40   # "enough" wherever the other arguments are what is wrong
    good = [p, 2, 0, 16, p, 4, p, p, 0, 64, p, p, p, ws, None, None]

    def but(**kw):
        names = ("recs", "world", "rank", "cap", "tab", "k", "residual", "out", "out_base", "out_len", "pay_idx",
                 "sel_gi", "ws", "ws_bytes", "status", "stream")
        a = list(good)
        for key, v in kw.items():
            a[names.index(key)] = v
        return tuple(a)
    return [but(recs=None), but(tab=None), but(residual=None), but(out=None), but(pay_idx=None), but(ws=None),
            but(world=0), but(world=1025, rank=0), but(cap=0), but(k=0), but(out_base=-1), but(out_len=-1),
            but(rank=2), but(rank=-1),
            but(world=1024, cap=1 << 21),          # world * cap = 2^31
            but(ws_bytes=16)]                      # shorter than grace_shard_select_workspace_bytes


@pytest.mark.parametrize("name", ["grace_shard_select", "grace_shard_select_bf16"])
def test_select_argument_errors_do_not_touch_the_device(name):
    from grace_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_uint32 * 64)()
    f = getattr(lib, name)
    for args in _bad_select_args(ctypes.addressof(buf)):
        assert f(*args) == -1, args
        assert lib.grace_last_error().startswith(name.encode() + b":"), lib.grace_last_error()


@pytest.mark.parametrize("name", ["grace_shard_clear", "grace_shard_clear_bf16"])
def test_clear_argument_errors_do_not_touch_the_device(name):
    from grace_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_uint32 * 64)()
    p = ctypes.addressof(buf)
    f = getattr(lib, name)
    for args in ((None, 0, 8, p, 8, None), (p, 0, 8, None, 8, None), (p, -1, 8, p, 8, None), (p, 0, -1, p, 8, None),
                 (p, 0, 8, p, -1, None)):
        assert f(*args) == -1, args
        assert lib.grace_last_error().startswith(name.encode() + b":"), lib.grace_last_error()
    assert f(p, 0, 8, p, 0, None) == 0     # nothing to clear: no launch


def test_fill_argument_errors_do_not_touch_the_device():
    from grace_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_uint32 * 64)()
    p = ctypes.addressof(buf)
    for args in ((None, 0, 8, None), (p, 0, -1, None), (p + 1, 0, 8, None)):   # null, n < 0, an odd address
        assert lib.grace_fill_bf16(*args) == -1, args
        assert lib.grace_last_error().startswith(b"grace_fill_bf16:"), lib.grace_last_error()
    assert lib.grace_fill_bf16(p, 0, 0, None) == 0   # n = 0: no launch


def test_out_dtype_is_checked_before_any_native_call(monkeypatch):
    from grace_amd import ops
    no_native(monkeypatch)
    i32 = torch.zeros(64, dtype=torch.int32)
    i64 = torch.zeros(4, dtype=torch.int64)
    res = torch.zeros(16)
    for dtype in (torch.float16, torch.float64, torch.int16):
        out = torch.zeros(32, dtype=dtype)
        with pytest.raises(TypeError):
            ops.shard_select(i32, 2, 0, 4, i64, 4, res, out, 0, i32[:4], i32[:1])
        with pytest.raises(TypeError):
            ops.shard_clear(out, 0, i32[:8])
    for dtype in (torch.float32, torch.bfloat16):    # a strided view is refused as well
        with pytest.raises(TypeError):
            ops.shard_clear(torch.zeros(32, dtype=dtype)[::2], 0, i32[:8])
    for bad in (torch.zeros(8), torch.zeros(8, dtype=torch.float16), torch.zeros(8, dtype=torch.bfloat16)[::2]):
        with pytest.raises(TypeError):
            ops.fill_bf16(bad)
    with pytest.raises(ops.GraceDeviceError):
        ops.fill_bf16(torch.zeros(8, dtype=torch.bfloat16))


def test_bf16_class_is_the_dist_class():
    from grace_amd.dist import sharded as S
    from grace_amd.sharded_bf16 import NativeShardKernels, ShardedTopK
    eng = ShardedTopK(0.01, dense="shard", check_sizes=True, recycle_output=False)
    assert isinstance(eng, S.ShardedTopK) and eng.dense == "shard" and eng.check_sizes and not eng.recycle_output
    assert isinstance(eng.k_ops, NativeShardKernels) and isinstance(eng.k_ops, S.NativeShardKernels)
    assert ShardedTopK.check is S.ShardedTopK.check
    marker = object()
    assert ShardedTopK(0.01, kernels=marker).k_ops is marker
    with pytest.raises(ValueError):
        ShardedTopK(0.01, dense="none")
    for dtype in (torch.float16, torch.float64, torch.int32):
        with pytest.raises(TypeError):
            eng.step(torch.zeros(100, dtype=dtype), "w")
