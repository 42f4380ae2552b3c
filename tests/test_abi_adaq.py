"""include/grace_hip_adaq.h is declared, exported and bound in _lib.SIGNATURES_ADAQ; the sizes follow the
header's formulas; bad arguments are refused without touching the device; and the Python layer validates on
the host before any native call.  No GPU is needed."""
import ctypes
import math

import pytest
import torch

from tests.abi_util import OnGpu, check_bad, check_types, declared, header, no_native

NAMES = ["grace_adaq_capacity", "grace_adaq_payload_bytes", "grace_adaq_workspace_bytes"] + [
    f + s for f in ("grace_adaq_compress", "grace_adaq_step_w1", "grace_adaq_decode_aggregate") for s in ("", "_bf16")]
SIZES = [(1, 1.0), (8192, 0.01), (8193, 0.3), (3 * 8192 + 5, 1.0), (100003, 0.017), (2 ** 31 - 1, 1.0)]


def want_sizes(n, ratio):
    cap = math.ceil(float(n) * ratio) + 4
    return cap, 16 + 16 * -(-(-(-n // 8192)) // 4) + 16 * -(-cap // 8)


def test_entry_points_declared_exported_bound():
    from grace_amd import _lib, ops
    hdr = header("grace_hip_adaq.h")
    assert declared(hdr) == sorted(NAMES) == sorted(_lib.SIGNATURES_ADAQ)
    check_types(hdr, _lib.SIGNATURES_ADAQ)
    raw, bound = ctypes.CDLL(_lib.LIB_PATH), _lib.load()
    for name, (res, args) in _lib.SIGNATURES_ADAQ.items():
        assert hasattr(raw, name), f"{name} is not exported by the library"
        f = getattr(bound, name)
        assert f.restype == res and list(f.argtypes) == args, name
        if name.endswith("_bf16"):
            assert _lib.SIGNATURES_ADAQ[name] == _lib.SIGNATURES_ADAQ[name[:-5]]
    cap, size, ws = bound.grace_adaq_capacity, bound.grace_adaq_payload_bytes, bound.grace_adaq_workspace_bytes
    for n, ratio in SIZES:
        assert (cap(n, ratio), size(n, ratio)) == want_sizes(n, ratio) == (ops.adaq_capacity(n, ratio),
                                                                            ops.adaq_payload_bytes(n, ratio))
    for n in (0, -1, 2 ** 31):
        assert cap(n, 0.5) == size(n, 0.5) == 0
    for ratio in (0.0, 1.5, -0.1, float("nan")):
        assert cap(4096, ratio) == size(4096, ratio) == 0
    assert ws(-1) == ws(2 ** 31) == 0 < ws(0) <= ws(1) < ws(2 ** 20) < ws(2 ** 31 - 1) and ws(1) % 16 == 0


def test_argument_errors_do_not_touch_the_device():
    """The pointers are host addresses: a launch would fault.  n == 0 is GRACE_OK with no launch."""
    from grace_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_uint64 * 64)()
    p = (ctypes.addressof(buf) + 15) & ~15
    q, w = p + 128, p + 256
    big = lib.grace_adaq_workspace_bytes(2 ** 20)
    for base in ("grace_adaq_compress", "grace_adaq_step_w1"):
        for name, odd in ((base, 2), (base + "_bf16", 1)):
            good = [p, 0, 0.5, q, w, big, None]          # x, n, ratio, payload or out, ws, ws_bytes, stream
            assert getattr(lib, name)(*good) == 0
            check_bad(lib, name, good, [(0, None), (3, None), (4, None), (0, p + odd), (4, w + 8),
                                        (3, q + (8 if "compress" in name else odd)), (1, -1), (1, 2 ** 31),
                                        (2, 0.0), (2, 1.5), (2, float("nan")), (5, 64)])
            check_bad(lib, name, [p, 2 ** 20, 0.5, q, w, big - 256, None], [(5, big - 256)])
    for name, odd in (("grace_adaq_decode_aggregate", 2), ("grace_adaq_decode_aggregate_bf16", 1)):
        good = [p, 32, 2, 0, 4, 2.0, q, None]            # payloads, stride, world, n, cap, divisor, out, stream
        assert getattr(lib, name)(*good) == 0
        check_bad(lib, name, good, [(0, None), (6, None), (0, p + 8), (6, q + odd), (1, 24), (1, -16), (2, 0), (2, 1025),
                                    (3, -1), (3, 2 ** 31), (4, -1), (4, 5), (5, 0.0)])
        stride = want_sizes(8193, 0.3)[1]                # shorter than the payload of (n, cap) by one line
        check_bad(lib, name, [p, stride - 16, 2, 8193, want_sizes(8193, 0.3)[0], 2.0, q, None], [(1, stride - 16)])


def test_host_validation_makes_no_native_call(monkeypatch):
    from grace_amd import ops
    from grace_amd.adaq import AdaqCompressor, grace_from_params
    from grace_amd.torch.compressor.adaq import AdaqCompressor as reexport
    no_native(monkeypatch)
    assert reexport is AdaqCompressor and AdaqCompressor().compress_ratio == 0.01
    assert AdaqCompressor(1).tensors_size_are_same
    for bad in (0, 1.5, -0.01, True, float("nan"), "0.1", None):
        with pytest.raises(ValueError):
            AdaqCompressor(bad)
        with pytest.raises(ValueError):
            grace_from_params({"compressor": "adaq", "compress_ratio": bad, "world_size": 1})
        with pytest.raises(ValueError):
            ops.adaq_capacity(4096, bad)
    f16 = torch.zeros(256, dtype=torch.float16).as_subclass(OnGpu)
    bf16 = torch.zeros(256, dtype=torch.bfloat16).as_subclass(OnGpu)
    pay = torch.zeros(256, dtype=torch.uint8).as_subclass(OnGpu)
    for call in (lambda: ops.adaq_compress(f16, 0.1), lambda: ops.adaq_step_w1(f16, 0.1),
                 lambda: AdaqCompressor(0.1).compress(bf16, "w"),
                 lambda: ops.adaq_decode_aggregate(pay, 2, 256, 0.1, out_dtype=torch.float16),
                 lambda: ops.adaq_decode_aggregate(pay.float(), 2, 256, 0.1)):
        with pytest.raises(TypeError) as e:
            call()
        assert not isinstance(e.value, ops.GraceDeviceError)
    for call in (lambda: ops.adaq_compress(torch.zeros(256), 0.1), lambda: AdaqCompressor(0.1).compress(torch.zeros(8), "w"),
                 lambda: ops.adaq_step_w1(torch.zeros(256, dtype=torch.bfloat16), 0.1),
                 lambda: ops.adaq_decode_aggregate(torch.zeros(256, dtype=torch.uint8), 2, 256, 0.1)):
        with pytest.raises(ops.GraceDeviceError):
            call()
    assert ops.adaq_payload_bytes(256, 0.1) == 96
    for call in (lambda: ops.adaq_decode_aggregate(pay, 0, 256, 0.1), lambda: ops.adaq_decode_aggregate(pay, 2, 256, 0.1, divisor=0),
                 lambda: ops.adaq_decode_aggregate(pay, 2, 256, 0.1, stride=104),     # no multiple of 16
                 lambda: ops.adaq_decode_aggregate(pay, 2, 256, 0.1, stride=144),     # past the buffer
                 lambda: ops.adaq_decode_aggregate(pay, 4, 256, 0.1),                 # 64 B a rank: shorter than the payload
                 lambda: ops.adaq_capacity(2 ** 31, 0.1), lambda: ops.adaq_payload_bytes(-1, 0.1)):
        with pytest.raises(ValueError):
            call()
