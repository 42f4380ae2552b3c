"""include/grace_hip_mx.h is declared, exported and bound in _lib.SIGNATURES_MX; the payload's size follows the
header's formula; bad arguments are refused without touching the device; and the Python layer validates on the
host before any native call.  No GPU is needed."""
import ctypes

import pytest
import torch

from tests.abi_util import OnGpu, check_bad, check_types, declared, header, no_native

NAMES = ["grace_mx_payload_bytes"] + [
    f + s for f in ("grace_mx_compress", "grace_mx_step_w1", "grace_mx_decode_aggregate") for s in ("", "_bf16")]
FORMATS = ("fp8_e4m3", "fp8_e5m2", "fp6_e2m3", "fp6_e3m2", "fp4_e2m1")
BITS = (8, 8, 6, 6, 4)


def want_bytes(n, f):
    nb = -(-n // 32)
    return 16 * -(-nb // 16) + 16 * -(-(nb * 4 * BITS[f]) // 16)


def test_entry_points_declared_exported_bound():
    from grace_amd import _lib, ops
    hdr = header("grace_hip_mx.h")
    assert declared(hdr) == sorted(NAMES) == sorted(_lib.SIGNATURES_MX)
    check_types(hdr, _lib.SIGNATURES_MX)
    raw, bound = ctypes.CDLL(_lib.LIB_PATH), _lib.load()
    for name, (res, args) in _lib.SIGNATURES_MX.items():
        assert hasattr(raw, name), f"{name} is not exported by the library"
        f = getattr(bound, name)
        assert f.restype == res and list(f.argtypes) == args, name
        if name.endswith("_bf16"):
            assert _lib.SIGNATURES_MX[name] == _lib.SIGNATURES_MX[name[:-5]]
    size = bound.grace_mx_payload_bytes
    assert (size(1, 0), size(32, 4), size(33, 2), size(33, 4)) == (48, 32, 64, 48)
    for n in (1, 32, 33, 511, 513, 100003, 2 ** 31 - 1):
        for f, fmt in enumerate(FORMATS):
            assert size(n, f) == want_bytes(n, f) == ops.mx_payload_bytes(n, fmt)
    for n, f in ((0, 0), (-1, 0), (2 ** 31, 0), (64, -1), (64, 5)):
        assert size(n, f) == 0


def test_argument_errors_do_not_touch_the_device():
    """The pointers are host addresses: a launch would fault.  n == 0 is GRACE_OK with no launch."""
    from grace_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_uint64 * 64)()
    p = (ctypes.addressof(buf) + 15) & ~15
    q, w = p + 128, p + 256
    for base in ("grace_mx_compress", "grace_mx_step_w1"):
        for name, odd in ((base, 2), (base + "_bf16", 1)):
            good = [p, 0, 4, 1, 7, w, q, None]             # x, n, format, rounding, seed, u, payload or out, stream
            assert getattr(lib, name)(*good) == 0
            assert getattr(lib, name)(p, 0, 0, 0, 7, None, q, None) == 0
            check_bad(lib, name, good, [(0, None), (6, None), (0, p + odd), (5, w + 2),
                                        (6, q + (8 if "compress" in name else odd)), (1, -1), (1, 2 ** 31),
                                        (2, -1), (2, 5), (3, -1), (3, 2)])
    for name, odd in (("grace_mx_decode_aggregate", 2), ("grace_mx_decode_aggregate_bf16", 1)):
        good = [p, 32, 2, 0, 4, 2.0, q, None]              # payloads, stride, world, n, format, divisor, out, stream
        assert getattr(lib, name)(*good) == 0
        check_bad(lib, name, good, [(0, None), (6, None), (0, p + 8), (6, q + odd), (1, 24), (1, -16), (2, 0), (2, 1025),
                                    (3, -1), (3, 2 ** 31), (4, -1), (4, 5), (5, 0.0)])
        stride = want_bytes(513, 2)                        # shorter than the payload by one line
        check_bad(lib, name, [p, stride - 16, 2, 513, 2, 2.0, q, None], [(1, stride - 16)])


def test_host_validation_makes_no_native_call(monkeypatch):
    from grace_amd import ops
    from grace_amd.dist.communicator.all_to_all import AllToAll
    from grace_amd.dist.memory.none import NoneMemory
    from grace_amd.mx import MXCompressor, grace_from_params
    from grace_amd.torch.compressor.mx import MXCompressor as reexport
    no_native(monkeypatch)
    comp = MXCompressor()
    assert reexport is MXCompressor and (comp.format, comp.rounding) == ("fp8_e4m3", "nearest")
    assert comp.tensors_size_are_same and ops.MX_FORMATS == FORMATS and ops.MX_BITS == BITS
    for bad in ("fp8", "FP4_E2M1", 0, None, True):
        with pytest.raises(ValueError):
            MXCompressor(bad)
        with pytest.raises(ValueError):
            MXCompressor("fp4_e2m1", bad)
        with pytest.raises(ValueError):
            grace_from_params({"compressor": "mx", "format": bad, "world_size": 1})
        with pytest.raises(ValueError):
            ops.mx_payload_bytes(4096, bad)
    f16 = torch.zeros(256, dtype=torch.float16).as_subclass(OnGpu)
    bf16 = torch.zeros(256, dtype=torch.bfloat16).as_subclass(OnGpu)
    f32 = torch.zeros(256).as_subclass(OnGpu)
    pay = torch.zeros(256, dtype=torch.uint8).as_subclass(OnGpu)
    for call in (lambda: ops.mx_compress(f16), lambda: ops.mx_step_w1(f16, "fp4_e2m1"),
                 lambda: MXCompressor().compress(bf16, "w"),
                 lambda: ops.mx_decode_aggregate(pay, 2, 64, "fp8_e4m3", out_dtype=torch.float16),
                 lambda: ops.mx_decode_aggregate(pay.float(), 2, 64, "fp8_e4m3")):
        with pytest.raises(TypeError) as e:
            call()
        assert not isinstance(e.value, ops.GraceDeviceError)
    for call in (lambda: ops.mx_compress(torch.zeros(256)), lambda: MXCompressor().compress(torch.zeros(8), "w"),
                 lambda: ops.mx_step_w1(torch.zeros(256, dtype=torch.bfloat16)),
                 lambda: ops.mx_compress(f32, rounding="stochastic", u=torch.zeros(256)),
                 lambda: ops.mx_decode_aggregate(torch.zeros(256, dtype=torch.uint8), 2, 64, "fp8_e4m3")):
        with pytest.raises(ops.GraceDeviceError):
            call()
    assert ops.mx_payload_bytes(64, "fp8_e4m3") == 80
    for call in (lambda: ops.mx_decode_aggregate(pay, 0, 64, "fp8_e4m3"),
                 lambda: ops.mx_decode_aggregate(pay, 2, 64, "fp8_e4m3", divisor=0),
                 lambda: ops.mx_decode_aggregate(pay, 2, 64, "fp8_e4m3", stride=88),      # no multiple of 16
                 lambda: ops.mx_decode_aggregate(pay, 2, 64, "fp8_e4m3", stride=144),     # past the buffer
                 lambda: ops.mx_decode_aggregate(pay, 4, 64, "fp8_e4m3"),                 # 64 B a rank: too short
                 lambda: ops.mx_compress(f32, rounding="stochastic", u=f32[:255]),
                 lambda: ops.mx_compress(f32, rounding="up"),
                 lambda: ops.mx_payload_bytes(2 ** 31, "fp8_e4m3"), lambda: ops.mx_payload_bytes(-1, "fp8_e4m3")):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(NotImplementedError):
        AllToAll(MXCompressor(), NoneMemory(), 2).step(f32, "w")
