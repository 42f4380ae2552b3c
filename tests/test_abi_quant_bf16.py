"""The entry points of include/grace_hip_quant.h are declared, exported and bound in
_lib.SIGNATURES_QUANT, mirror their f32 forms and refuse bad arguments without touching the device;
the first two headers and tables are what they were.  The dtype and limit checks of the ops wrappers
and the class relations of grace_amd.quant_bf16 need no GPU either."""
import ctypes
import os
import re

import pytest
import torch

from tests.abi_util import ROOT, OnGpu, check_bad, declared, header, no_native, params

# f32 form -> its parameters that become uint16_t* in the twin
TWINS = {
    "grace_qsgd_compress_at": ("const float* x",),
    "grace_qsgd_step_w1": ("const float* x", "float* out"),
    "grace_qsgd_decompress": ("float* out",),
    "grace_terngrad_compress": ("const float* x",),
    "grace_terngrad_step_w1": ("const float* x", "float* out"),
    "grace_terngrad_decompress": ("float* out",),
}
NEW = tuple(sorted(f + "_bf16" for f in TWINS))


def test_entry_points_declared_exported_bound():
    from grace_amd import _lib
    quant = header("grace_hip_quant.h")
    assert '#include "grace_hip.h"' in quant and 'extern "C"' in quant
    assert declared(quant) == sorted(NEW) == sorted(_lib.SIGNATURES_QUANT)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert hasattr(lib, name), f"{name} is not exported by the library"
    bound = _lib.load()
    for name, (res, args) in _lib.SIGNATURES_QUANT.items():
        f = getattr(bound, name)
        assert f.restype == res and list(f.argtypes) == args, name
        assert len(args) == params(quant, name).count(",") + 1, name
    raw = open(os.path.join(ROOT, "include", "grace_hip_quant.h")).read()
    for name in NEW:   # a doc comment right above every entry point
        assert re.search(r"\*/\s*\n[a-z_ ]+\b%s\(" % name, raw), f"{name} has no doc comment"


def test_first_two_headers_and_tables_are_unchanged():
    from grace_amd import _lib
    names = declared(header("grace_hip.h"))
    assert len(names) == 159 and len(_lib.SIGNATURES) == 159 and sorted(_lib.SIGNATURES) == names
    sign = declared(header("grace_hip_sign.h"))
    assert len(sign) == 11 and len(_lib.SIGNATURES_SIGN) == 11 and sorted(_lib.SIGNATURES_SIGN) == sign
    for table in (names, sign, _lib.SIGNATURES, _lib.SIGNATURES_SIGN):
        assert not set(NEW) & set(table)


@pytest.mark.parametrize("f32", sorted(TWINS))
def test_bf16_twin_mirrors_the_f32_entry_point(f32):
    from grace_amd import _lib
    want = params(header("grace_hip.h"), f32)
    for s in TWINS[f32]:
        assert want.count(s) == 1, (f32, s)
        want = want.replace(s, s.replace("float*", "uint16_t*"))
    assert params(header("grace_hip_quant.h"), f32 + "_bf16") == want
    assert _lib.SIGNATURES_QUANT[f32 + "_bf16"] == _lib.SIGNATURES[f32]


def test_argument_errors_do_not_touch_the_device():
    """A null required pointer, a negative size, world < 1, bucket_size != 128, nseg past the limit
    and an odd address return -1 with "name: ..."; an empty input is GRACE_OK.  The pointers are host
    addresses: a launch would fault."""
    from grace_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_uint64 * 64)()
    p = ctypes.addressof(buf)
    assert p % 8 == 0
    seg_max = lib.grace_qsgd_seg_max()
    assert seg_max == 512

    # x, xoff, seg_off, bkt_off, nseg, nbuckets, q, bucket_size, variant, u, seed, norms_in, norms_out, codes, stream
    name = "grace_qsgd_compress_at_bf16"
    good = [p, 0, p, p, 1, 4, 127, 128, 0, None, 1, None, p, p, None]
    bad = [(0, None), (2, None), (3, None), (12, None), (13, None), (0, p + 1), (0, p + 2), (0, p + 4), (1, -1),
           (4, 0), (4, seg_max + 1), (5, -1), (5, 1 << 24), (6, 0), (7, 64), (7, 256), (8, 2)]
    check_bad(lib, name, good, bad)
    check_bad(lib, name, [p, 0, p, p, 1, 4, 255, 128, 1, None, 1, None, p, p, None], [(6, 255)])   # variant 1: q < 128
    good[5] = 0
    assert getattr(lib, name)(*good) == 0

    # x, seg_off, bkt_off, nseg, nbuckets, q, variant, u, seed, out, stream
    name = "grace_qsgd_step_w1_bf16"
    good = [p, p, p, 1, 4, 127, 0, None, 1, p, None]
    bad = [(0, None), (1, None), (2, None), (9, None), (0, p + 2), (9, p + 2), (9, p + 1), (3, 0), (3, seg_max + 1),
           (4, -1), (4, 1 << 24), (5, 0), (6, 3)]
    check_bad(lib, name, good, bad)
    good[4] = 0
    assert getattr(lib, name)(*good) == 0

    # codes, norms, code_stride, norm_stride, world, seg_off, bkt_off, nseg, n, q, bucket_size, variant, agg, div, out, stream
    name = "grace_qsgd_decompress_bf16"
    good = [p, p, 512, 4, 2, p, p, 1, 512, 127, 128, 0, 1, 2.0, p, None]
    bad = [(0, None), (1, None), (5, None), (6, None), (14, None), (14, p + 2), (4, 0), (4, -1), (7, 0),
           (7, seg_max + 1), (8, -1), (8, 1 << 31), (10, 64), (9, 0)]
    check_bad(lib, name, good, bad)
    good[8] = 0
    assert getattr(lib, name)(*good) == 0

    # x, seg_off, unit_off, nseg, nunits, clip_in, u, seed, codes, scalars, ws, stream
    name = "grace_terngrad_compress_bf16"
    good = [p, p, p, 1, 1, None, None, 1, p, p, p, None]
    bad = [(0, None), (1, None), (2, None), (8, None), (9, None), (10, None), (0, p + 2), (6, p + 8), (3, 0),
           (3, seg_max + 1), (4, 0), (4, -1), (4, (1 << 17) + 2)]
    check_bad(lib, name, good, bad)

    # x, seg_off, unit_off, nseg, nunits, clip_in, u, seed, scalars, ws, out, stream
    name = "grace_terngrad_step_w1_bf16"
    good = [p, p, p, 1, 1, None, None, 1, p, p, p, None]
    bad = [(0, None), (1, None), (2, None), (8, None), (9, None), (10, None), (0, p + 2), (10, p + 2), (10, p + 1),
           (6, p + 4), (3, 0), (3, seg_max + 1), (4, 0), (4, -1), (4, (1 << 17) + 2)]
    check_bad(lib, name, good, bad)

    # codes, scalars, code_stride, scal_stride, world, seg_off, nseg, n, aggregate, divisor, out, stream
    name = "grace_terngrad_decompress_bf16"
    good = [p, p, 512, 1, 2, p, 1, 512, 1, 2.0, p, None]
    bad = [(0, None), (1, None), (5, None), (10, None), (10, p + 2), (10, p + 4), (4, 0), (4, -2), (6, 0),
           (6, seg_max + 1), (7, -1), (7, 1 << 31)]
    check_bad(lib, name, good, bad)
    good[7] = 0
    assert getattr(lib, name)(*good) == 0


def test_ops_check_dtypes_before_any_native_call(monkeypatch):
    from grace_amd import ops
    no_native(monkeypatch)
    i8, f32 = torch.zeros(256, dtype=torch.int8), torch.zeros(2)
    for dtype in (torch.float16, torch.float64, torch.int16):
        for x in (torch.zeros(256, dtype=dtype), torch.zeros(256, dtype=dtype).as_subclass(OnGpu)):
            for call in (lambda: ops.qsgd_compress(x, 127, 128), lambda: ops.qsgd_step_w1(x, 127),
                         lambda: ops.terngrad_compress(x), lambda: ops.terngrad_step_w1(x),
                         lambda: ops.qsgd_decompress(i8, f32, 127, 128, 256, out_dtype=dtype),
                         lambda: ops.terngrad_decompress(i8, f32[:1], 256, out_dtype=dtype)):
                with pytest.raises(TypeError) as e:
                    call()
                assert not isinstance(e.value, ops.GraceDeviceError), dtype   # the dtype check comes first
    # accepted dtypes on the CPU get as far as the device check, still without a native call
    for dtype in (torch.float32, torch.bfloat16):
        x = torch.zeros(256, dtype=dtype)
        for call in (lambda: ops.qsgd_compress(x, 127, 128), lambda: ops.qsgd_step_w1(x, 127),
                     lambda: ops.terngrad_compress(x), lambda: ops.terngrad_step_w1(x)):
            with pytest.raises(ops.GraceDeviceError):
                call()
    for out_dtype in (torch.float32, torch.bfloat16):
        with pytest.raises(ops.GraceDeviceError):
            ops.qsgd_decompress(i8, f32, 127, 128, 256, out_dtype=out_dtype)
        with pytest.raises(ops.GraceDeviceError):
            ops.terngrad_decompress(i8, f32[:1], 256, out_dtype=out_dtype)


def test_ops_refuse_bf16_outside_the_fast_paths(monkeypatch):
    """bucket_size != 128, more than 512 segments, 2^24 buckets or more, 2^31 elements or more and
    a misaligned bf16 view: ValueError before any native call (CPU and `meta` tensors)."""
    from grace_amd import ops
    no_native(monkeypatch)
    x = torch.zeros(1024, dtype=torch.bfloat16)
    many = [2] * 513
    xm = torch.zeros(1026, dtype=torch.bfloat16)
    for call in (lambda: ops.qsgd_compress(x, 127, 64), lambda: ops.qsgd_compress(x, 127, 256),
                 lambda: ops.qsgd_compress(xm, 127, 128, sizes=many), lambda: ops.qsgd_step_w1(xm, 127, sizes=many),
                 lambda: ops.terngrad_compress(xm, sizes=many), lambda: ops.terngrad_step_w1(xm, sizes=many)):
        with pytest.raises(ValueError):
            call()
    big = torch.empty(1 << 31, dtype=torch.bfloat16, device="meta")
    for call in (lambda: ops.qsgd_compress(big, 127, 128), lambda: ops.qsgd_step_w1(big, 127),
                 lambda: ops.terngrad_compress(big), lambda: ops.terngrad_step_w1(big)):
        with pytest.raises(ValueError):
            call()
    i8, f32 = torch.zeros(1026, dtype=torch.int8), torch.zeros(513)
    for call in (lambda: ops.qsgd_decompress(i8, f32, 127, 64, 1024, out_dtype=torch.bfloat16),
                 lambda: ops.qsgd_decompress(i8, f32, 127, 128, 1026, sizes=many, out_dtype=torch.bfloat16),
                 lambda: ops.terngrad_decompress(i8, f32, 1026, sizes=many, out_dtype=torch.bfloat16),
                 lambda: ops.terngrad_decompress(i8, f32, 1 << 31, out_dtype=torch.bfloat16)):
        with pytest.raises(ValueError):
            call()
    # alignment: a view that starts on an odd element (as if it were on the GPU)
    monkeypatch.setattr(ops, "dev_grad", lambda t, what="gradient": t)
    odd = torch.zeros(1025, dtype=torch.bfloat16)[1:]
    assert odd.data_ptr() % 8
    for call in (lambda: ops.qsgd_compress(odd, 127, 128), lambda: ops.qsgd_step_w1(odd, 127),
                 lambda: ops.terngrad_compress(odd), lambda: ops.terngrad_step_w1(odd)):
        with pytest.raises(ValueError):
            call()


def test_classes_are_the_dist_classes():
    from grace_amd import quant_bf16 as Q
    from grace_amd.dist.compressor.qsgd import QSGDCompressor, QSGDCompressor_CUDA
    from grace_amd.dist.compressor.terngrad import TernGradCompressor
    for new, old in ((Q.QSGDCompressor, QSGDCompressor), (Q.QSGDCompressor_CUDA, QSGDCompressor_CUDA),
                     (Q.TernGradCompressor, TernGradCompressor)):
        assert issubclass(new, old) and new is not old
        # only fused_step is overridden
        for attr in ("compress", "decompress", "decode_aggregate_gathered", "_uniforms", "a2a_decode_sum", "__init__"):
            assert getattr(new, attr) is getattr(old, attr), (new, attr)
        assert new.fused_step is not old.fused_step
    assert not issubclass(Q.QSGDCompressor, QSGDCompressor_CUDA)
    c = Q.QSGDCompressor(127, 128, rng="torch_cpu")
    assert (c.quantum_num, c.bucket_size, c.rng, c.variant, c.average) == (127, 128, "torch_cpu", 0, True)
    assert Q.QSGDCompressor_CUDA(127).variant == 1 and Q.QSGDCompressor(255).bucket_size == 128
    t = Q.TernGradCompressor(rng="torch_cpu", wire="2bit")
    assert (t.rng, t.wire) == ("torch_cpu", "2bit")
    with pytest.raises(ValueError):
        Q.TernGradCompressor(wire="u4")


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_compress_by_hand_still_refuses(dtype):
    """compress is the parent's: bf16 (and float16) raise TypeError, so AllToAll and ResidualMemory
    keep refusing bf16; so does the Allgather step on a tensor that is not on the GPU."""
    from grace_amd import quant_bf16 as Q
    from grace_amd.dist.communicator.allgather import Allgather
    from grace_amd.dist.memory.none import NoneMemory
    x = torch.zeros(256, dtype=dtype)
    for comp in (Q.QSGDCompressor(127), Q.QSGDCompressor_CUDA(127), Q.TernGradCompressor()):
        for t in (x, x.as_subclass(OnGpu)):
            with pytest.raises(TypeError):
                comp.compress(t, "w")
        with pytest.raises(TypeError):
            Allgather(comp, NoneMemory(), 1).step(x, "w")
