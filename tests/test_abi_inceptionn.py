"""include/grace_hip_inceptionn.h is declared, exported and bound in _lib.SIGNATURES_INCEPTIONN; bad arguments
are refused without touching the device; and the Python layer validates on the host before any native call.
No GPU is needed."""
import ctypes

import pytest
import torch

from tests.abi_util import OnGpu, check_bad, check_types, declared, header, no_native

NAMES = ["grace_inceptionn_capacity_bytes"] + [
    f + s for f in ("grace_inceptionn_compress", "grace_inceptionn_step_w1", "grace_inceptionn_decode_aggregate")
    for s in ("", "_bf16")]


def test_entry_points_declared_exported_bound():
    from grace_amd import _lib
    hdr = header("grace_hip_inceptionn.h")
    assert declared(hdr) == sorted(NAMES) == sorted(_lib.SIGNATURES_INCEPTIONN)
    check_types(hdr, _lib.SIGNATURES_INCEPTIONN)
    raw, bound = ctypes.CDLL(_lib.LIB_PATH), _lib.load()
    for name, (res, args) in _lib.SIGNATURES_INCEPTIONN.items():
        assert hasattr(raw, name), f"{name} is not exported by the library"
        f = getattr(bound, name)
        assert f.restype == res and list(f.argtypes) == args, name
        if name.endswith("_bf16"):
            assert _lib.SIGNATURES_INCEPTIONN[name] == _lib.SIGNATURES_INCEPTIONN[name[:-5]]
    size = bound.grace_inceptionn_capacity_bytes
    # the header (word 0 and a word a tile, padded to 16 B) plus 16 ceil(m / 64) + 16 ceil(m / 4) bytes a tile
    assert [size(n) for n in (1, 64, 65, 4096, 4097, 3 * 4096)] == [48, 288, 320, 16 + 17408, 16 + 17408 + 32,
                                                                     16 + 3 * 17408]
    assert size(4 * 4096) == 32 + 4 * 17408 and size(0) == size(-1) == size(2 ** 31) == 0


def test_argument_errors_do_not_touch_the_device():
    """The pointers are host addresses: a launch would fault.  n == 0 is GRACE_OK with no launch."""
    from grace_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_uint64 * 64)()
    p = (ctypes.addressof(buf) + 15) & ~15
    q = p + 128
    shape = [(1, -1), (1, 2 ** 31), (2, 0), (2, 15)]
    for base in ("grace_inceptionn_compress", "grace_inceptionn_step_w1"):
        for name, odd in ((base, 2), (base + "_bf16", 1)):
            good = [p, 0, 10, q, None]                   # x, n, b, payload or out, stream
            assert getattr(lib, name)(*good) == 0
            check_bad(lib, name, good, [(0, None), (3, None), (0, p + odd), (3, q + (8 if "compress" in name else odd))]
                      + shape)
    for name, odd in (("grace_inceptionn_decode_aggregate", 2), ("grace_inceptionn_decode_aggregate_bf16", 1)):
        good = [p, 32, 2, 0, 10, 2.0, q, None]           # payloads, stride, world, n, b, divisor, out, stream
        assert getattr(lib, name)(*good) == 0
        check_bad(lib, name, good, [(0, None), (6, None), (0, p + 8), (6, q + odd), (1, 24), (1, -16), (2, 0), (2, 1025),
                                    (3, -1), (3, 2 ** 31), (4, 0), (4, 15), (5, 0.0)])
        check_bad(lib, name, [p, 16, 2, 3 * 4096 + 1, 10, 2.0, q, None], [(1, 16)])   # five words of header in 16 bytes


def test_host_validation_makes_no_native_call(monkeypatch):
    from grace_amd import ops
    from grace_amd.inceptionn import InceptionnCompressor, grace_from_params
    from grace_amd.torch.compressor.inceptionn import InceptionnCompressor as reexport
    no_native(monkeypatch)
    assert reexport is InceptionnCompressor and InceptionnCompressor().bound_bits == 10
    assert not InceptionnCompressor(14).tensors_size_are_same
    for bad in (0, 15, -1, True, 10.0, "10"):
        with pytest.raises(ValueError):
            InceptionnCompressor(bad)
        with pytest.raises(ValueError):
            grace_from_params({"compressor": "inceptionn", "bound_bits": bad, "world_size": 1})
    f16 = torch.zeros(256, dtype=torch.float16).as_subclass(OnGpu)
    bf16 = torch.zeros(256, dtype=torch.bfloat16).as_subclass(OnGpu)
    pay = torch.zeros(256, dtype=torch.uint8).as_subclass(OnGpu)
    for call in (lambda: ops.inceptionn_compress(f16, 10), lambda: ops.inceptionn_step_w1(f16, 10),
                 lambda: InceptionnCompressor(10).compress(bf16, "w"),
                 lambda: ops.inceptionn_decode_aggregate(pay, 2, 256, 10, out_dtype=torch.float16),
                 lambda: ops.inceptionn_decode_aggregate(pay.float(), 2, 256, 10)):
        with pytest.raises(TypeError) as e:
            call()
        assert not isinstance(e.value, ops.GraceDeviceError)
    for call in (lambda: ops.inceptionn_compress(torch.zeros(256), 10),
                 lambda: InceptionnCompressor(10).compress(torch.zeros(8), "w"),
                 lambda: ops.inceptionn_step_w1(torch.zeros(256, dtype=torch.bfloat16), 10),
                 lambda: ops.inceptionn_decode_aggregate(torch.zeros(256, dtype=torch.uint8), 2, 256, 10)):
        with pytest.raises(ops.GraceDeviceError):
            call()
    for call in (lambda: ops.inceptionn_decode_aggregate(pay, 0, 256, 10),
                 lambda: ops.inceptionn_decode_aggregate(pay, 2, 256, 10, divisor=0),
                 lambda: ops.inceptionn_decode_aggregate(pay, 2, 256, 10, stride=136),     # no multiple of 16
                 lambda: ops.inceptionn_decode_aggregate(pay, 2, 256, 10, stride=144),     # past the buffer
                 lambda: ops.inceptionn_decode_aggregate(pay, 16, 3 * 4096 + 1, 10),       # shorter than the header
                 lambda: ops.inceptionn_capacity_bytes(2 ** 31)):
        with pytest.raises(ValueError):
            call()


def test_all_to_all_refuses_the_codec():
    from grace_amd.dist.communicator.all_to_all import AllToAll
    from grace_amd.dist.memory.none import NoneMemory
    from grace_amd.inceptionn import InceptionnCompressor
    with pytest.raises(NotImplementedError):
        AllToAll(InceptionnCompressor(10), NoneMemory(), 2).send_receive([], "w", (torch.float32, torch.Size([8])))
