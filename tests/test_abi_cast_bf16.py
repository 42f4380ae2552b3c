"""The entry points of include/grace_hip_cast.h are declared, exported and bound in
_lib.SIGNATURES_CAST, every `_bf16` twin mirrors its f32 form, bad arguments are refused without
touching the device, and the first five headers and tables are what they were.  The dtype checks of
the ops wrappers and the class relations of grace_amd.cast_bf16 need no GPU either."""
import ctypes
import os
import re

import pytest
import torch

from tests.abi_util import ROOT, OnGpu, check_bad, check_types, declared, header, no_native, params

# twin -> (the header of its f32 form, the parameters that become uint16_t*)
TWINS = {
    "grace_natural_compress_at_bf16": ("grace_hip.h", ("const float* x",)),
    "grace_cnat_compress_at_bf16": ("grace_hip.h", ("const float* x",)),
    "grace_fp16_compress_bf16": ("grace_hip.h", ("const float* x",)),
    "grace_cast_step_w1_bf16": ("grace_hip.h", ("const float* x", "float* out")),
    "grace_natural_decompress_bf16": ("grace_hip.h", ("float* out",)),
    "grace_fp16_decompress_aggregate_bf16": ("grace_hip.h", ("float* out",)),
    "grace_onebit_encode_bf16": ("grace_hip.h", ("const float* x",)),
    "grace_onebit_step_w1_bf16": ("grace_hip_cast.h", ("const float* x", "float* out")),
    "grace_onebit_decode_aggregate_bf16": ("grace_hip_cast.h", ("float* out",)),
}
NEW = tuple(TWINS) + ("grace_onebit_step_w1", "grace_onebit_decode_aggregate")


def test_entry_points_declared_exported_bound():
    from grace_amd import _lib
    hdr = header("grace_hip_cast.h")
    assert '#include "grace_hip.h"' in hdr and 'extern "C"' in hdr
    assert declared(hdr) == sorted(NEW) == sorted(_lib.SIGNATURES_CAST)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert hasattr(lib, name), f"{name} is not exported by the library"
    bound = _lib.load()
    for name, (res, args) in _lib.SIGNATURES_CAST.items():
        f = getattr(bound, name)
        assert f.restype == res and list(f.argtypes) == args, name
        assert res is _lib.ST
    check_types(hdr, _lib.SIGNATURES_CAST)      # each bound type is the prototype's
    raw = open(os.path.join(ROOT, "include", "grace_hip_cast.h")).read()
    for name in NEW:   # a doc comment above every entry point or above the f32 form of its pair
        first = name[:-5] if name.endswith("_bf16") and name[:-5] in NEW else name
        assert re.search(r"\*/\s*\n[a-z_ ]+\b%s\(" % first, raw), f"{name} has no doc comment"


def test_first_five_headers_and_tables_are_unchanged():
    from grace_amd import _lib
    for h, table, count in (("grace_hip.h", _lib.SIGNATURES, 159), ("grace_hip_sign.h", _lib.SIGNATURES_SIGN, 11),
                            ("grace_hip_quant.h", _lib.SIGNATURES_QUANT, 6),
                            ("grace_hip_dgc.h", _lib.SIGNATURES_DGC, 8),
                            ("grace_hip_sparse.h", _lib.SIGNATURES_SPARSE, 7)):
        names = declared(header(h))
        assert len(names) == count and len(table) == count and sorted(table) == names, h
        assert not set(NEW) & set(names)


@pytest.mark.parametrize("twin", sorted(TWINS))
def test_twin_mirrors_the_f32_entry_point(twin):
    from grace_amd import _lib
    src, changed = TWINS[twin]
    f32 = twin[:-5]
    want = params(header(src), f32)
    for s in changed:
        assert want.count(s) == 1, s
        want = want.replace(s, s.replace("float*", "uint16_t*"))
    assert params(header("grace_hip_cast.h"), twin) == want
    table = _lib.SIGNATURES if src == "grace_hip.h" else _lib.SIGNATURES_CAST
    assert _lib.SIGNATURES_CAST[twin] == table[f32]


def test_argument_errors_do_not_touch_the_device():
    """A null required pointer, a negative size, a bad mode / flavour / world and an address the entry
    point cannot use at all return -1 with "name: ..."; an empty input is GRACE_OK where stated.  The
    pointers are host addresses: a launch would fault."""
    from grace_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_uint64 * 64)()
    p = ctypes.addressof(buf)
    q, r, s = p + 64, p + 128, p + 192
    assert p % 8 == 0

    # x, xoff, n, rand, seed, codes, stream
    for name in ("grace_natural_compress_at_bf16",):
        good = [p, 0, 0, None, 7, q, None]
        assert getattr(lib, name)(*good) == 0
        check_bad(lib, name, good, [(0, None), (5, None), (2, -1), (1, -4), (1, 2), (0, p + 1), (3, r + 2)])
    # x, xoff, n, rand, deterministic, seed, codes, stream
    good = [p, 0, 0, None, 0, 7, q, None]
    assert lib.grace_cnat_compress_at_bf16(*good) == 0
    check_bad(lib, "grace_cnat_compress_at_bf16", good,
              [(0, None), (6, None), (2, -1), (1, -4), (1, 6), (0, p + 1), (3, r + 2)])
    # x, half_out, n, stream
    good = [p, q, 0, None]
    assert lib.grace_fp16_compress_bf16(*good) == 0
    check_bad(lib, "grace_fp16_compress_bf16", good, [(0, None), (1, None), (2, -1), (0, p + 1), (1, q + 1)])
    # x, n, mode, seed, out, stream
    good = [p, 0, 0, 7, q, None]
    assert lib.grace_cast_step_w1_bf16(*good) == 0
    check_bad(lib, "grace_cast_step_w1_bf16", good,
              [(0, None), (4, None), (1, -1), (2, -1), (2, 4), (0, p + 1), (4, q + 1)])
    # codes, stride, world, n, flavour, aggregate, divisor, out, stream
    good = [p, 0, 1, 0, 0, 1, 1.0, q, None]
    assert lib.grace_natural_decompress_bf16(*good) == 0
    check_bad(lib, "grace_natural_decompress_bf16", good,
              [(0, None), (7, None), (3, -1), (2, 0), (2, -1), (4, 2), (4, -1), (6, 0.0), (7, q + 1)])
    good = [p, 8, 2, 16, 0, 1, 2.0, q, None]
    check_bad(lib, "grace_natural_decompress_bf16", good, [(1, 15)])           # rows that overlap
    # half_in, stride, world, n, divisor, out, stream
    good = [p, 0, 1, 0, 1.0, q, None]
    assert lib.grace_fp16_decompress_aggregate_bf16(*good) == 0
    check_bad(lib, "grace_fp16_decompress_aggregate_bf16", good,
              [(0, None), (5, None), (3, -1), (2, 0), (2, -1), (4, 0.0), (0, p + 1), (5, q + 1)])
    good = [p, 16, 2, 16, 2.0, q, None]
    check_bad(lib, "grace_fp16_decompress_aggregate_bf16", good, [(1, 15)])

    # x, n, mask0, means, ws, stream
    good = [p, 16, q, r, s, None]
    check_bad(lib, "grace_onebit_encode_bf16", good,
              [(0, None), (2, None), (3, None), (4, None), (1, 0), (1, -1), (0, p + 1), (3, r + 2), (4, s + 4)])
    # x, n, quirk, means, out, ws, stream
    good = [p, 16, 0, r, q, s, None]
    for name, odd in (("grace_onebit_step_w1", 2), ("grace_onebit_step_w1_bf16", 1)):
        check_bad(lib, name, good, [(0, None), (3, None), (4, None), (5, None), (1, 0), (1, -1), (0, p + odd),
                                    (4, q + odd), (3, r + 2), (5, s + 4)])
    # mask0_wn, mean0_w, mean1_w, world, quirk, divisor, out, n, stream
    good = [p, q, r, 2, 0, 2.0, s, 0, None]
    for name, odd in (("grace_onebit_decode_aggregate", 2), ("grace_onebit_decode_aggregate_bf16", 1)):
        assert getattr(lib, name)(*good) == 0
        check_bad(lib, name, good, [(0, None), (1, None), (2, None), (6, None), (3, 0), (3, -1), (5, 0.0), (7, -1),
                                    (6, s + odd), (1, q + 2)])


def test_ops_check_dtypes_before_any_native_call(monkeypatch):
    from grace_amd import ops
    no_native(monkeypatch)
    bf = torch.zeros(256, dtype=torch.bfloat16).as_subclass(OnGpu)
    u8 = torch.zeros(512, dtype=torch.uint8).as_subclass(OnGpu)
    f16 = torch.zeros(512, dtype=torch.float16).as_subclass(OnGpu)
    m = torch.zeros(2).as_subclass(OnGpu)
    for dtype in (torch.float16, torch.float64, torch.int16):
        x = torch.zeros(256, dtype=dtype).as_subclass(OnGpu)
        for call in (lambda: ops.natural_compress(x), lambda: ops.cnat_compress(x), lambda: ops.fp16_compress(x),
                     lambda: ops.onebit_encode_grad(x), lambda: ops.onebit_step_w1(x)):
            with pytest.raises(TypeError) as e:
                call()
            assert not isinstance(e.value, ops.GraceDeviceError), dtype
        for call in (lambda: ops.natural_decompress(u8, 256, 0, world=2, aggregate=True, out_dtype=dtype),
                     lambda: ops.fp16_decompress_aggregate(f16, 256, 2, out_dtype=dtype),
                     lambda: ops.onebit_decode_aggregate(u8, m, m, 2, 256, out_dtype=dtype)):
            with pytest.raises(TypeError):
                call()
    cpu = torch.zeros(256, dtype=torch.bfloat16)             # not on the GPU: the device check
    for call in (lambda: ops.natural_compress(cpu), lambda: ops.cnat_compress(cpu), lambda: ops.fp16_compress(cpu),
                 lambda: ops.cast_step_w1(cpu, 3, 0), lambda: ops.onebit_encode_grad(cpu), lambda: ops.onebit_step_w1(cpu)):
        with pytest.raises(ops.GraceDeviceError):
            call()
    # injected randoms of a bf16 encode: the dtype, the length and the device; xoff a multiple of 4
    ri = torch.zeros(256, dtype=torch.int32).as_subclass(OnGpu)
    for bad in (ri.float(), ri[:255], torch.zeros(512, dtype=torch.int32)[::2].as_subclass(OnGpu)):
        with pytest.raises(TypeError):
            ops.natural_compress(bf, rand_int=bad)
    for bad in (ri, torch.zeros(255).as_subclass(OnGpu)):
        with pytest.raises(TypeError):
            ops.cnat_compress(bf, rand=bad)
    with pytest.raises(ValueError):
        ops.natural_compress(bf, rand_int=torch.zeros(256, dtype=torch.int32))           # on the CPU
    for call in (lambda: ops.natural_compress(bf, xoff=2), lambda: ops.cnat_compress(bf, xoff=-4),
                 lambda: ops.cast_step_w1(bf, 4, 0), lambda: ops.cast_step_w1(bf, -1, 0),
                 lambda: ops.onebit_step_w1(bf[:0]), lambda: ops.onebit_encode_grad(bf[:0])):
        with pytest.raises(ValueError):
            call()
    # gathered payloads of a bf16 decode: the dtype and world * n elements
    for call in (lambda: ops.natural_decompress(u8, 255, 0, world=2, aggregate=True, out_dtype=torch.bfloat16),
                 lambda: ops.natural_decompress(f16, 256, 0, world=2, aggregate=True, out_dtype=torch.bfloat16),
                 lambda: ops.fp16_decompress_aggregate(f16, 255, 2, out_dtype=torch.bfloat16),
                 lambda: ops.fp16_decompress_aggregate(u8, 256, 2, out_dtype=torch.bfloat16),
                 lambda: ops.onebit_decode_aggregate(u8, m, m, 2, 255),
                 lambda: ops.onebit_decode_aggregate(u8, m, m[:1], 2, 256),
                 lambda: ops.onebit_decode_aggregate(f16, m, m, 2, 256)):
        with pytest.raises(TypeError):
            call()
    for call in (lambda: ops.natural_decompress(u8, 256, 2, world=2, aggregate=True, out_dtype=torch.bfloat16),
                 lambda: ops.natural_decompress(u8, 256, 0, world=0, aggregate=True, out_dtype=torch.bfloat16),
                 lambda: ops.fp16_decompress_aggregate(f16, 256, 2, divisor=0.0, out_dtype=torch.bfloat16),
                 lambda: ops.onebit_decode_aggregate(u8, m, m, 0, 256),
                 lambda: ops.onebit_decode_aggregate(u8, m, m, 2, 256, divisor=0)):
        with pytest.raises(ValueError):
            call()


def test_f32_calls_reach_the_same_entry_points_with_the_same_arguments(monkeypatch):
    from grace_amd import _lib, ops
    calls = []
    monkeypatch.setattr(_lib, "call", lambda name, *a: calls.append((name, a)))
    monkeypatch.setattr(_lib, "query", lambda name, *a: 4096)
    monkeypatch.setattr(ops, "_stream", lambda: 99)
    monkeypatch.setattr(ops, "workspace", lambda slot, nbytes, device: None)
    monkeypatch.setattr(torch, "empty", lambda *a, device=None, **kw: torch.zeros(*a, **kw).as_subclass(OnGpu))
    monkeypatch.setattr(torch, "empty_like", lambda t, **kw: torch.zeros(t.shape, dtype=t.dtype).as_subclass(OnGpu))
    x = torch.zeros(64).as_subclass(OnGpu)
    u8 = torch.zeros(128, dtype=torch.uint8).as_subclass(OnGpu)
    f16 = torch.zeros(128, dtype=torch.float16).as_subclass(OnGpu)
    ops.natural_compress(x, seed=-1, xoff=8)
    ops.cnat_compress(x, deterministic=True)
    ops.fp16_compress(x)
    ops.cast_step_w1(x, 1, 5)
    ops.natural_decompress(u8, 64, 1, world=2, aggregate=True, divisor=2)
    ops.fp16_decompress_aggregate(f16, 64, 2, divisor=2)
    ops.onebit_encode(x)
    ops.onebit_encode_grad(x)
    names = [c[0] for c in calls]
    assert names == ["grace_natural_compress_at", "grace_cnat_compress_at", "grace_fp16_compress", "grace_cast_step_w1",
                     "grace_natural_decompress", "grace_fp16_decompress_aggregate", "grace_onebit_encode",
                     "grace_onebit_encode"]
    px = x.data_ptr()
    assert calls[0][1][:5] == (px, 8, 64, None, 2 ** 64 - 1) and calls[0][1][6] == 99
    assert calls[1][1][:6] == (px, 0, 64, None, 1, 0)
    assert calls[2][1][0] == px and calls[2][1][2:] == (64, 99)
    assert calls[3][1][:4] == (px, 64, 1, 5)
    assert calls[4][1][:7] == (u8.data_ptr(), 64, 2, 64, 1, 1, 2.0)
    assert calls[5][1][:5] == (f16.data_ptr(), 64, 2, 64, 2.0)
    assert calls[6][1][:2] == (px, 64) and calls[6][1][4:] == (None, 99)
    # ... and the same calls on bfloat16 reach the twins
    calls.clear()
    bf = torch.zeros(64, dtype=torch.bfloat16).as_subclass(OnGpu)
    ops.natural_compress(bf)
    ops.cnat_compress(bf)
    ops.fp16_compress(bf)
    ops.cast_step_w1(bf, 3, 0)
    ops.natural_decompress(u8, 64, 1, world=2, aggregate=True, divisor=2, out_dtype=torch.bfloat16)
    ops.fp16_decompress_aggregate(f16, 64, 2, divisor=2, out_dtype=torch.bfloat16)
    ops.onebit_encode_grad(bf)
    ops.onebit_step_w1(bf)
    assert [c[0] for c in calls] == [
        "grace_natural_compress_at_bf16", "grace_cnat_compress_at_bf16", "grace_fp16_compress_bf16",
        "grace_cast_step_w1_bf16", "grace_natural_decompress_bf16", "grace_fp16_decompress_aggregate_bf16",
        "grace_onebit_encode_bf16", "grace_onebit_step_w1_bf16"]


def test_classes_are_the_dist_classes():
    from grace_amd import cast_bf16 as C
    from grace_amd.dist.compressor.fp16 import FP16Compressor
    from grace_amd.dist.compressor.natural import NaturalCompressor, NaturalCompressor_CUDA
    from grace_amd.dist.compressor.onebit import OneBitCompressor
    for ours, parent in ((C.NaturalCompressor, NaturalCompressor), (C.NaturalCompressor_CUDA, NaturalCompressor_CUDA),
                         (C.FP16Compressor, FP16Compressor), (C.OneBitCompressor, OneBitCompressor)):
        assert issubclass(ours, parent) and ours is not parent
        for attr in ("compress", "decompress", "__init__", "aggregate"):
            assert getattr(ours, attr) is getattr(parent, attr), (ours, attr)
        assert ours.fused_step is not parent.fused_step
    assert C.NaturalCompressor_CUDA._encode is NaturalCompressor_CUDA._encode
    assert C.NaturalCompressor_CUDA.flavour == 1 and C.NaturalCompressor.flavour == 0
    c = C.NaturalCompressor_CUDA(rng="deterministic")
    assert (c.rng, c._step, c._w1_mode()) == ("deterministic", 0, 2)
    assert C.OneBitCompressor(compat_uint8_not=True).compat_uint8_not is True


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_by_hand_still_refuses(dtype):
    """compress is the parents': bf16 and float16 raise TypeError by hand and under ResidualMemory, and
    so does the Allgather step on a tensor that is not on the GPU; grace_amd.dist's own classes keep
    refusing bf16 on the Allgather step."""
    from grace_amd import cast_bf16 as C
    from grace_amd.dist.communicator.allgather import Allgather
    from grace_amd.dist.compressor.fp16 import FP16Compressor
    from grace_amd.dist.compressor.natural import NaturalCompressor, NaturalCompressor_CUDA
    from grace_amd.dist.compressor.onebit import OneBitCompressor
    from grace_amd.dist.memory.none import NoneMemory
    from grace_amd.dist.memory.residual import ResidualMemory
    x = torch.zeros(256, dtype=dtype)
    gpu = x.as_subclass(OnGpu)
    for comp in (C.NaturalCompressor(), C.NaturalCompressor_CUDA(), C.FP16Compressor(), C.OneBitCompressor()):
        with pytest.raises(TypeError):
            comp.compress(gpu, "w")
        for mem in (NoneMemory(), ResidualMemory()):
            if isinstance(comp, FP16Compressor):      # off the GPU it hands any tensor through, as the reference does
                continue
            with pytest.raises(TypeError):
                Allgather(comp, mem, 1).step(x, "w")
        with pytest.raises(TypeError):
            Allgather(comp, ResidualMemory(), 1).step(gpu, "w")
    for comp in (NaturalCompressor(), NaturalCompressor_CUDA(), FP16Compressor(), OneBitCompressor()):
        with pytest.raises(TypeError):
            Allgather(comp, NoneMemory(), 1).step(gpu, "w")
