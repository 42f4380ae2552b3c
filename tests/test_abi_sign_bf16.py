"""The entry points of include/grace_hip_sign.h are declared, exported and bound in
_lib.SIGNATURES_SIGN, mirror their f32 forms and refuse bad arguments without touching the device;
include/grace_hip.h and _lib.SIGNATURES are what they were.  The dtype checks of the ops wrappers
and the class relations of grace_amd.sign_bf16 need no GPU either."""
import ctypes
import os
import re

import pytest
import torch

from tests.abi_util import ROOT, OnGpu, check_bad, declared, header, no_native, params

NEW = ("grace_efsign_workspace_bytes", "grace_efsign_step", "grace_efsign_step_bf16",
       "grace_efsign_decode_aggregate", "grace_efsign_decode_aggregate_bf16", "grace_sign_encode_bf16",
       "grace_sign_encode_bits_bf16", "grace_sign_step_w1_bf16", "grace_sign_majority_bf16",
       "grace_sign_majority_bits_bf16", "grace_signum_encode_bf16")
# f32 form -> (the header that declares it, its parameters that become uint16_t* in the twin)
TWINS = {
    "grace_efsign_step": ("grace_hip_sign.h", ("const float* g", "float* out")),
    "grace_efsign_decode_aggregate": ("grace_hip_sign.h", ("float* out",)),
    "grace_sign_encode": ("grace_hip.h", ("const float* x",)),
    "grace_sign_encode_bits": ("grace_hip.h", ("const float* x",)),
    "grace_sign_step_w1": ("grace_hip.h", ("const float* x", "float* out")),
    "grace_sign_majority": ("grace_hip.h", ("float* out",)),
    "grace_sign_majority_bits": ("grace_hip.h", ("float* out",)),
    "grace_signum_encode": ("grace_hip.h", ("const float* g",)),
}


def test_entry_points_declared_exported_bound():
    from grace_amd import _lib
    sign = header("grace_hip_sign.h")
    assert '#include "grace_hip.h"' in sign and 'extern "C"' in sign
    assert declared(sign) == sorted(NEW) == sorted(_lib.SIGNATURES_SIGN)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert hasattr(lib, name), f"{name} is not exported by the library"
    bound = _lib.load()
    for name, (res, args) in _lib.SIGNATURES_SIGN.items():
        f = getattr(bound, name)
        assert f.restype == res and list(f.argtypes) == args, name
        assert len(args) == params(sign, name).count(",") + 1, name
    # every entry point of the new header has a doc comment right above it
    raw = open(os.path.join(ROOT, "include", "grace_hip_sign.h")).read()
    for name in NEW:
        assert re.search(r"\*/\s*\n[a-z_ ]+\b%s\(" % name, raw), f"{name} has no doc comment"


def test_first_header_and_table_are_unchanged():
    from grace_amd import _lib
    names = declared(header("grace_hip.h"))
    assert len(names) == 159 and len(_lib.SIGNATURES) == 159 and sorted(_lib.SIGNATURES) == names
    assert not set(NEW) & set(names) and not set(NEW) & set(_lib.SIGNATURES)


@pytest.mark.parametrize("f32", sorted(TWINS))
def test_bf16_twin_mirrors_the_f32_entry_point(f32):
    from grace_amd import _lib
    where, subs = TWINS[f32]
    want = params(header(where), f32)
    for s in subs:
        assert want.count(s) == 1, (f32, s)
        want = want.replace(s, s.replace("float*", "uint16_t*"))
    assert params(header("grace_hip_sign.h"), f32 + "_bf16") == want
    table = _lib.SIGNATURES if where == "grace_hip.h" else _lib.SIGNATURES_SIGN
    assert _lib.SIGNATURES_SIGN[f32 + "_bf16"] == table[f32]


@pytest.mark.parametrize("bf16", [False, True])
def test_argument_errors_do_not_touch_the_device(bf16):
    """A null required pointer, n < 0, world < 1, a short workspace and (bf16) an odd address return
    -1 with "name: ..."; n == 0 is GRACE_OK.  The pointers are host addresses: a launch would fault."""
    from grace_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_uint32 * 64)()
    p = ctypes.addressof(buf)
    sfx = "_bf16" if bf16 else ""
    odd = [p + 1] if bf16 else []
    ws = lib.grace_efsign_workspace_bytes(1000)
    assert ws >= 8 and lib.grace_efsign_workspace_bytes(1 << 30) <= 1 << 20

    # g, residual, has, lr_mem, n, mean_out, codes, out, lr_agg, ws, ws_bytes, stream
    name = "grace_efsign_step" + sfx
    good = [p, p, 1, 0.1, 8, p, None, None, 0.1, p, ws, None]
    bad = [(0, None), (1, None), (5, None), (9, None), (4, -1), (10, ws - 1), (10, 0)]
    bad += [(0, a) for a in odd] + [(7, a) for a in odd]
    check_bad(lib, name, good, bad)
    good[4] = 0
    assert getattr(lib, name)(*good) == 0

    name = "grace_efsign_decode_aggregate" + sfx      # means, codes_wn, world, lr_agg, out, n, stream
    good = [p, p, 2, 0.1, p, 8, None]
    check_bad(lib, name, good, [(0, None), (1, None), (4, None), (2, 0), (2, -3), (5, -1)] + [(4, a) for a in odd])
    good[5] = 0
    assert getattr(lib, name)(*good) == 0

    if not bf16:
        return
    cases = {
        "grace_sign_encode_bf16": ([p, p, 8, None], [(0, None), (1, None), (2, -1), (0, p + 1)], 2),
        "grace_sign_encode_bits_bf16": ([p, 8, p, None], [(0, None), (2, None), (1, -1), (0, p + 1)], 1),
        "grace_sign_step_w1_bf16": ([p, None, p, 8, None], [(0, None), (2, None), (3, -1), (0, p + 1), (2, p + 1)], 3),
        "grace_sign_majority_bf16": ([p, 2, p, 8, None], [(0, None), (2, None), (1, 0), (3, -1), (2, p + 1)], 3),
        "grace_sign_majority_bits_bf16": ([p, 1, 2, 8, p, None],
                                          [(0, None), (4, None), (2, 0), (2, 64), (3, -1), (4, p + 1)], 3),
        "grace_signum_encode_bf16": ([p, p, 1, 0.5, 0.5, p, 8, None],
                                     [(0, None), (1, None), (5, None), (6, -1), (0, p + 1)], 6),
    }
    for name, (good, bad, n_at) in cases.items():
        check_bad(lib, name, good, bad)
        good[n_at] = 0
        assert getattr(lib, name)(*good) == 0, name


def test_ops_check_dtypes_before_any_native_call(monkeypatch):
    from grace_amd import ops
    no_native(monkeypatch)
    u8 = torch.zeros(64, dtype=torch.uint8)
    for dtype in (torch.float16, torch.float64, torch.int16):
        x = torch.zeros(64, dtype=dtype).as_subclass(OnGpu)
        assert x.device.type == "cuda" and x.dtype == dtype
        f32 = torch.zeros(64)
        for call in (lambda: ops.sign_encode(x), lambda: ops.sign_encode_bits(x), lambda: ops.sign_step_w1(x),
                     lambda: ops.signum_encode(x, f32, True, 0.9),
                     lambda: ops.efsign_step(x, f32, True, 0.1, 0.1, want_codes=True),
                     lambda: ops.sign_majority(u8, 1, 64, out_dtype=dtype),
                     lambda: ops.sign_majority_bits(torch.zeros(2, dtype=torch.int32), 1, 64, out_dtype=dtype),
                     lambda: ops.efsign_decode_aggregate(f32[:1], u8, 1, 64, 0.1, out_dtype=dtype)):
            with pytest.raises(TypeError) as e:
                call()
            assert not isinstance(e.value, ops.GraceDeviceError), dtype   # the dtype check comes first
    # accepted dtypes on the CPU get as far as the device check, still without a native call
    for dtype in (torch.float32, torch.bfloat16):
        x = torch.zeros(64, dtype=dtype)
        for call in (lambda: ops.sign_encode(x), lambda: ops.sign_encode_bits(x), lambda: ops.sign_step_w1(x),
                     lambda: ops.signum_encode(x, torch.zeros(64), True, 0.9),
                     lambda: ops.efsign_step(x, torch.zeros(64), True, 0.1, 0.1, want_codes=True)):
            with pytest.raises(ops.GraceDeviceError):
                call()


def test_ops_check_shapes_before_any_native_call(monkeypatch):
    """efsign_step's residual and out, signum_encode's momentum on bf16, and the decode's payload
    sizes: checked on `meta` tensors, which have a device type of their own and no memory."""
    from grace_amd import ops
    no_native(monkeypatch)
    monkeypatch.setattr(ops, "dev_grad", lambda t, what="gradient": t)   # as if the tensors were on the GPU
    monkeypatch.setattr(ops, "require_dev", lambda t, what="tensor": t)
    g = torch.zeros(64, dtype=torch.bfloat16)
    for res in (torch.zeros(63), torch.zeros(64, dtype=torch.bfloat16), torch.zeros(128)[::2], None):
        with pytest.raises(TypeError):
            ops.efsign_step(g, res, True, 0.1, 0.1, want_codes=False)
        with pytest.raises(TypeError):
            ops.signum_encode(g, res, True, 0.9)
    for out in (torch.zeros(64), torch.zeros(63, dtype=torch.bfloat16), torch.zeros(128, dtype=torch.bfloat16)[::2]):
        with pytest.raises(ValueError):
            ops.efsign_step(g, torch.zeros(64), True, 0.1, 0.1, want_codes=False, out=out)
    with pytest.raises(ValueError):    # an f32 step's result is f32
        ops.efsign_step(torch.zeros(64), torch.zeros(64), True, 0.1, 0.1, want_codes=False, out=g)
    u8 = torch.zeros(128, dtype=torch.uint8)
    for means, codes, world in ((torch.zeros(1), u8, 2), (torch.zeros(2), u8[:100], 2), (torch.zeros(2), u8.int(), 2),
                                (torch.zeros(2, dtype=torch.float64), u8, 2)):
        with pytest.raises(TypeError):
            ops.efsign_decode_aggregate(means, codes, world, 64, 0.1)
    with pytest.raises(ValueError):
        ops.efsign_decode_aggregate(torch.zeros(0), u8[:0], 0, 64, 0.1)


def test_classes_are_the_dist_classes():
    from grace_amd import sign_bf16 as S
    from grace_amd.dist.compressor.efsignsgd import EFSignSGDCompressor
    from grace_amd.dist.compressor.signsgd import SignSGDCompressor
    from grace_amd.dist.compressor.signum import SignumCompressor
    assert issubclass(S.SignSGDCompressor, SignSGDCompressor) and S.SignSGDCompressor is not SignSGDCompressor
    assert issubclass(S.SignumCompressor, SignumCompressor) and S.SignumCompressor is not SignumCompressor
    assert issubclass(S.EFSignSGDCompressor, EFSignSGDCompressor) and S.EFSignSGDCompressor is not EFSignSGDCompressor
    assert S.SignSGDCompressor(wire="bits").wire == "bits" and not S.SignSGDCompressor().average
    with pytest.raises(ValueError):
        S.SignSGDCompressor(wire="u4")
    assert S.SignumCompressor(0.9).momentum == 0.9 and S.SignumCompressor(0.9).momentums == {}
    assert S.EFSignSGDCompressor(0.25).learning_rate == 0.25
    # what the subclasses do not redefine is the parent's
    assert S.SignSGDCompressor.compress is SignSGDCompressor.compress
    assert S.EFSignSGDCompressor.compress is EFSignSGDCompressor.compress
    assert S.SignumCompressor.decompress is SignumCompressor.decompress


@pytest.mark.parametrize("dtype", [torch.float16, torch.float64])
def test_other_dtypes_are_refused(dtype):
    """float16 / float64 through every class and the Allgather step: TypeError (tests/
    test_gpu_sign_bf16_dist.py repeats it with float16 on the GPU)."""
    from grace_amd import sign_bf16 as S
    from grace_amd.dist.communicator.allgather import Allgather
    from grace_amd.dist.memory.efsignsgd import EFSignSGDMemory
    from grace_amd.dist.memory.none import NoneMemory
    x = torch.zeros(100, dtype=dtype)
    for comm in (Allgather(S.SignSGDCompressor(), NoneMemory(), 1),
                 Allgather(S.SignSGDCompressor("bits"), NoneMemory(), 1),
                 Allgather(S.SignumCompressor(0.9), NoneMemory(), 1),
                 Allgather(S.EFSignSGDCompressor(0.1), EFSignSGDMemory(0.1), 1)):
        with pytest.raises(TypeError):
            comm.step(x, "w")
