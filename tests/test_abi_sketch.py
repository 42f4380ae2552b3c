"""include/grace_hip_sketch.h is declared, exported and bound in _lib.SIGNATURES_SKETCH; bad arguments are
refused without touching the device; and the Python layer validates on the host before any native call.
No GPU is needed."""
import ctypes

import pytest
import torch

from tests.abi_util import OnGpu, check_bad, check_types, declared, header, no_native

NAMES = ["grace_sketch_workspace_bytes"] + [
    f + s for f in ("grace_sketch_edges", "grace_sketch_compress", "grace_sketch_step_w1",
                    "grace_sketch_decode_aggregate") for s in ("", "_bf16")]


def test_entry_points_declared_exported_bound():
    from grace_amd import _lib
    hdr = header("grace_hip_sketch.h")
    assert declared(hdr) == sorted(NAMES) == sorted(_lib.SIGNATURES_SKETCH)
    check_types(hdr, _lib.SIGNATURES_SKETCH)
    raw, bound = ctypes.CDLL(_lib.LIB_PATH), _lib.load()
    for name, (res, args) in _lib.SIGNATURES_SKETCH.items():
        assert hasattr(raw, name), f"{name} is not exported by the library"
        f = getattr(bound, name)
        assert f.restype == res and list(f.argtypes) == args, name
        if name.endswith("_bf16"):
            assert _lib.SIGNATURES_SKETCH[name] == _lib.SIGNATURES_SKETCH[name[:-5]]
    size = bound.grace_sketch_workspace_bytes
    assert size(10, 17) - size(0, 17) == 10 and size(11, 16) - size(0, 16) == 6 and size(0, 2) > 0
    assert size(-1, 16) == size(2 ** 31, 16) == size(8, 1) == size(8, 257) == 0


def test_argument_errors_do_not_touch_the_device():
    """The pointers are host addresses: a launch would fault.  n == 0 is GRACE_OK with no launch."""
    from grace_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_uint64 * 64)()
    p = ctypes.addressof(buf)
    q, r, s = p + 64, p + 128, p + 192
    shape = [(1, -1), (1, 2 ** 31), (2, 1), (2, 257)]
    for name, odd in (("grace_sketch_edges", 2), ("grace_sketch_edges_bf16", 1)):
        good = [p, 0, 16, q, r, None]                  # x, n, q, edges, ws, stream
        assert getattr(lib, name)(*good) == 0
        check_bad(lib, name, good, [(0, None), (3, None), (4, None), (0, p + odd), (3, q + 2), (4, r + 4)] + shape)
    for base in ("grace_sketch_compress", "grace_sketch_step_w1"):
        for name, odd in ((base, 2), (base + "_bf16", 1)):
            good = [p, 0, 256, q, r, s, None]          # x, n, q, means, codes or out, ws, stream
            assert getattr(lib, name)(*good) == 0
            bad = [(0, None), (3, None), (4, None), (5, None), (0, p + odd), (3, q + 2), (5, s + 4)] + shape
            check_bad(lib, name, good, bad + ([(4, r + odd)] if "step" in name else []))
    for name, odd in (("grace_sketch_decode_aggregate", 2), ("grace_sketch_decode_aggregate_bf16", 1)):
        good = [p, 0, q, 2, 0, 16, 2.0, r, None]       # codes, stride, means, world, n, q, divisor, out, stream
        assert getattr(lib, name)(*good) == 0
        check_bad(lib, name, good, [(0, None), (2, None), (7, None), (3, 0), (3, 1025), (4, -1), (5, 1), (5, 257),
                                    (6, 0.0), (7, r + odd), (2, q + 2)])
        check_bad(lib, name, [p, 8, q, 2, 16, 16, 2.0, r, None], [(1, 7)])      # rows that overlap
        check_bad(lib, name, [p, 16, q, 2, 16, 17, 2.0, r, None], [(1, 15)])


def test_host_validation_makes_no_native_call(monkeypatch):
    from grace_amd import ops
    from grace_amd.sketch import SketchCompressor, grace_from_params
    from grace_amd.torch.compressor.sketch import SketchCompressor as reexport
    no_native(monkeypatch)
    assert reexport is SketchCompressor and SketchCompressor(256).quantiles == 256
    for bad in (1, 257, 0, True, 16.0, "16"):
        with pytest.raises(ValueError):
            SketchCompressor(bad)
        with pytest.raises(ValueError):
            grace_from_params({"compressor": "sketch", "quantiles": bad, "world_size": 1})
    f16 = torch.zeros(256, dtype=torch.float16).as_subclass(OnGpu)
    bf16 = torch.zeros(256, dtype=torch.bfloat16).as_subclass(OnGpu)
    codes, means = torch.zeros(256, dtype=torch.uint8).as_subclass(OnGpu), torch.zeros(32).as_subclass(OnGpu)
    for call in (lambda: ops.sketch_edges(f16, 16), lambda: ops.sketch_compress(f16, 16),
                 lambda: ops.sketch_step_w1(f16, 16), lambda: SketchCompressor(16).compress(bf16, "w"),
                 lambda: ops.sketch_decode_aggregate(codes, means, 2, 256, 16, out_dtype=torch.float16),
                 lambda: ops.sketch_decode_aggregate(codes.float(), means, 2, 256, 16),
                 lambda: ops.sketch_decode_aggregate(codes, means, 2, 256, 17)):     # 17 buckets: a byte a code
        with pytest.raises(TypeError) as e:
            call()
        assert not isinstance(e.value, ops.GraceDeviceError)
    for call in (lambda: ops.sketch_compress(torch.zeros(256), 16), lambda: SketchCompressor(16).compress(torch.zeros(8), "w"),
                 lambda: ops.sketch_step_w1(torch.zeros(256, dtype=torch.bfloat16), 16)):
        with pytest.raises(ops.GraceDeviceError):
            call()
    for call in (lambda: ops.sketch_decode_aggregate(codes, means, 0, 256, 16),
                 lambda: ops.sketch_decode_aggregate(codes, means, 2, 256, 16, divisor=0),
                 lambda: ops.sketch_decode_aggregate(codes, means, 2, 256, 16, code_stride=100),
                 lambda: ops.sketch_edges(bf16[:0], 16)):
        with pytest.raises(ValueError):
            call()


def test_all_to_all_refuses_the_codec():
    from grace_amd.dist.communicator.all_to_all import AllToAll
    from grace_amd.dist.memory.none import NoneMemory
    from grace_amd.sketch import SketchCompressor
    with pytest.raises(NotImplementedError):
        AllToAll(SketchCompressor(16), NoneMemory(), 2).send_receive([], "w", (torch.float32, torch.Size([8])))
