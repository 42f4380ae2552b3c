"""include/grace_hip_u8bit.h is declared, exported and bound in _lib.SIGNATURES_U8BIT; bad arguments are
refused without touching the device; the default tables are what DESIGN.md §15 says; and the Python
layer validates on the host before any native call.  No GPU is needed."""
import ctypes

import pytest
import torch

from tests.abi_util import OnGpu, check_bad, check_types, declared, header, no_native

NAMES = [f + s for f in ("grace_u8bit_compress", "grace_u8bit_step_w1", "grace_u8bit_decode_aggregate")
         for s in ("", "_bf16")]


def test_entry_points_declared_exported_bound():
    from grace_amd import _lib
    hdr = header("grace_hip_u8bit.h")
    assert declared(hdr) == sorted(NAMES) == sorted(_lib.SIGNATURES_U8BIT)
    check_types(hdr, _lib.SIGNATURES_U8BIT)
    raw, bound = ctypes.CDLL(_lib.LIB_PATH), _lib.load()
    for name, (res, args) in _lib.SIGNATURES_U8BIT.items():
        assert hasattr(raw, name), f"{name} is not exported by the library"
        f = getattr(bound, name)
        assert f.restype is _lib.ST and f.restype == res and list(f.argtypes) == args, name
        if name.endswith("_bf16"):
            assert _lib.SIGNATURES_U8BIT[name] == _lib.SIGNATURES_U8BIT[name[:-5]]


def test_argument_errors_do_not_touch_the_device():
    """The pointers are host addresses: a launch would fault.  n == 0 is GRACE_OK with no launch."""
    from grace_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_uint64 * 64)()
    p = ctypes.addressof(buf)
    q, r, s, t = p + 64, p + 128, p + 192, p + 256
    blocks = [(2, 100), (2, 128), (2, 8192), (2, -256), (2, 768)]
    for name, odd in (("grace_u8bit_compress", 2), ("grace_u8bit_compress_bf16", 1)):
        good = [p, 0, 256, q, r, s, None, None]        # x, n, block, edges, scales, codes, ws, stream
        assert getattr(lib, name)(*good) == 0
        check_bad(lib, name, good, [(0, None), (3, None), (4, None), (5, None), (1, -1), (0, p + odd)] + blocks)
        good[2], good[6] = 0, t                         # tensor-wide: the workspace is required
        assert getattr(lib, name)(*good) == 0
        check_bad(lib, name, good, [(6, None)])
    for name, odd in (("grace_u8bit_step_w1", 2), ("grace_u8bit_step_w1_bf16", 1)):
        good = [p, 0, 4096, q, r, s, t, None, None]    # x, n, block, edges, values, scales, out, ws, stream
        assert getattr(lib, name)(*good) == 0
        check_bad(lib, name, good, [(0, None), (3, None), (4, None), (5, None), (6, None), (1, -1), (0, p + odd),
                                    (6, t + odd)] + blocks)
        good[2] = 0
        check_bad(lib, name, good, [(7, None)])
    for name, odd in (("grace_u8bit_decode_aggregate", 2), ("grace_u8bit_decode_aggregate_bf16", 1)):
        good = [p, 0, q, 2, 0, 512, r, 2.0, s, None]   # codes, stride, scales, world, n, block, values, divisor, out
        assert getattr(lib, name)(*good) == 0
        check_bad(lib, name, good, [(0, None), (2, None), (6, None), (8, None), (3, 0), (3, -1), (3, 1025), (4, -1),
                                    (7, 0.0), (8, s + odd), (5, 100), (5, 8192)])
        check_bad(lib, name, [p, 15, q, 2, 16, 512, r, 2.0, s, None], [(1, 15)])     # rows that overlap


@pytest.mark.parametrize("rounding", ["floor", "nearest"])
def test_default_tables(rounding):
    from grace_amd import ops
    edges, values = ops.u8bit_host_tables(rounding)
    for t in (edges, values):
        assert t.dtype == torch.float32 and t.shape == (128,) and bool((t[1:] > t[:-1]).all())
    assert values[0] == 0 and values[127] == 1 and edges[0] == 0
    assert float(values[1]) == pytest.approx(3.25e-6) and float(values[126]) == pytest.approx(0.1 + 0.9 * 127 / 128)
    if rounding == "floor":
        assert torch.equal(edges, values)
    else:
        assert bool((edges[1:] > values[:-1]).all()) and bool((edges[1:] < values[1:]).all())


def test_host_validation_makes_no_native_call(monkeypatch):
    from grace_amd import ops
    from grace_amd.u8bit import U8bitCompressor, grace_from_params
    no_native(monkeypatch)
    good = torch.linspace(0, 1, 128)
    assert U8bitCompressor(512, "nearest", good.tolist()).block_size == 512
    swapped = good.clone()
    swapped[[5, 6]] = swapped[[6, 5]]
    for book in (swapped, good[:127], good - 0.5, good.tolist() + [float("inf")], "abc", good.to(torch.int32)):
        with pytest.raises(ValueError):
            U8bitCompressor(codebook=book)
    for kw in ({"block_size": 100}, {"block_size": 8192}, {"rounding": "up"}):
        with pytest.raises(ValueError):
            U8bitCompressor(**kw)
    with pytest.raises(ValueError):
        grace_from_params({"compressor": "u8bit", "block_size": 100, "world_size": 1})
    table = torch.zeros(128).as_subclass(OnGpu)
    f16 = torch.zeros(256, dtype=torch.float16).as_subclass(OnGpu)
    codes, scales = torch.zeros(512, dtype=torch.int8).as_subclass(OnGpu), torch.zeros(2).as_subclass(OnGpu)
    for call in (lambda: ops.u8bit_compress(f16, 256, table), lambda: ops.u8bit_step_w1(f16, 0, table, table),
                 lambda: ops.u8bit_compress(f16.float(), 256, table[:127]),
                 lambda: ops.u8bit_decode_aggregate(codes, scales, 2, 256, 256, table, out_dtype=torch.float16),
                 lambda: ops.u8bit_decode_aggregate(codes.float(), scales, 2, 256, 256, table),
                 lambda: ops.u8bit_decode_aggregate(codes, scales[:1], 2, 256, 256, table)):
        with pytest.raises(TypeError) as e:
            call()
        assert not isinstance(e.value, ops.GraceDeviceError)
    for call in (lambda: ops.u8bit_compress(torch.zeros(256), 256, table),
                 lambda: ops.u8bit_step_w1(torch.zeros(256, dtype=torch.bfloat16), 256, table, table)):
        with pytest.raises(ops.GraceDeviceError):
            call()
    for call in (lambda: ops.u8bit_compress(f16.float(), 100, table),
                 lambda: ops.u8bit_decode_aggregate(codes, scales, 0, 256, 256, table),
                 lambda: ops.u8bit_decode_aggregate(codes, scales, 2, 256, 256, table, divisor=0)):
        with pytest.raises(ValueError):
            call()


def test_all_to_all_refuses_the_codec():
    """AllToAll serves the codecs that name a kind; this one does not, and says so before any exchange."""
    from grace_amd.dist.communicator.all_to_all import AllToAll
    from grace_amd.dist.memory.none import NoneMemory
    from grace_amd.u8bit import U8bitCompressor
    with pytest.raises(NotImplementedError):
        AllToAll(U8bitCompressor(), NoneMemory(), 2).send_receive([], "w", (torch.float32, torch.Size([8])))
