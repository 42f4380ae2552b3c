"""grace_sparse_aggregate_sorted_bf16 is declared, exported and bound, mirrors the f32 entry point and
refuses bad arguments without touching the device; the Python pieces of the bf16 Allgather step that
need no GPU (ops.sparse_aggregate_sorted's out_dtype check, grace_amd.topk_bf16's class)."""
import ctypes
import re

import pytest
import torch

from tests.abi_util import header

NAME = "grace_sparse_aggregate_sorted_bf16"


def test_entry_point_declared_exported_bound():
    from grace_amd import _lib
    hdr = header("grace_hip.h")
    m = re.search(r"\b%s\s*\(([^)]*)\)" % NAME, hdr)
    assert m, "not declared in include/grace_hip.h"
    f32 = re.search(r"\bgrace_sparse_aggregate_sorted\s*\(([^)]*)\)", hdr).group(1)
    squeeze = lambda s: re.sub(r"\s+", " ", s).strip()
    assert squeeze(m.group(1)) == squeeze(f32).replace("float* out", "uint16_t* out")
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), NAME), "not exported by the library"
    assert _lib.SIGNATURES[NAME] == _lib.SIGNATURES["grace_sparse_aggregate_sorted"]


def test_argument_errors_do_not_touch_the_device():
    from grace_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_uint32 * 8)()
    p = ctypes.addressof(buf)
    for args in ((None, None, None, 4, 1, 1.0, None, 8, None),       # null pointers
                 (p, p, p, 4, 0, 1.0, p, 8, None),                   # world < 1
                 (p, p, p, 4, 1025, 1.0, p, 8, None),                # world > 1024
                 (p, p, p, 4, 1, 1.0, p, 0, None),                   # n < 1
                 (p, p, p, 4, 1, 1.0, p, (1 << 28) + 1, None)):      # n > 2^28
        assert lib.grace_sparse_aggregate_sorted_bf16(*args) == -1, args
        assert NAME.encode() in lib.grace_last_error()


def test_out_dtype_is_checked_before_anything_is_allocated():
    from grace_amd import ops
    g = torch.zeros(16)
    for dtype in (torch.float16, torch.float64, torch.int16):
        with pytest.raises(TypeError):
            ops.sparse_aggregate_sorted(g, 1, 1, 4, 1, out_dtype=dtype)


def test_bf16_compressor_is_the_dist_compressor_and_has_no_cpu_path():
    from grace_amd.dist.compressor.topk import TopKCompressor as F32TopK
    from grace_amd.ops import GraceDeviceError
    from grace_amd.topk_bf16 import TopKCompressor
    c = TopKCompressor(0.01, recycle_output="always", check_sync=True)
    assert isinstance(c, F32TopK) and c.recycle_output == "always" and c.check_sync
    assert TopKCompressor.decompress is F32TopK.decompress and TopKCompressor.fused_step is F32TopK.fused_step
    for dtype in (torch.float32, torch.bfloat16):
        with pytest.raises(GraceDeviceError):
            c.compress(torch.zeros(100, dtype=dtype), "w")
