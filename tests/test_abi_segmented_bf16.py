"""The bfloat16 segmented top-k entry points are declared in include/grace_hip.h, exported by the
library and bound in grace_amd/_lib.py; the chunk queries return the main pass's chunk lengths of
both element types; bad arguments are refused without touching the device (no GPU)."""
import ctypes
import re

import pytest

from tests.abi_util import header

NAMES = ["grace_topk_segmented_chunk_bf16", "grace_topk_segmented_step_bf16"]
# (has_residual, dense_out): elements per main-pass chunk
CASES = [(1, 1), (1, 0), (0, 1), (0, 0)]


@pytest.mark.parametrize("name", NAMES)
def test_segmented_bf16_entry_point_declared_exported_bound(name):
    from grace_amd import _lib
    hdr = header("grace_hip.h")
    assert re.search(r"\b%s\s*\(" % name, hdr), "not declared in include/grace_hip.h"
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name), "not exported by the library"
    assert name in _lib.SIGNATURES, "not bound in grace_amd/_lib.py"


def test_segmented_bf16_twins_mirror_f32_signatures():
    """g and out change type only (all pointers in the binding)."""
    from grace_amd._lib import SIGNATURES as S
    assert S["grace_topk_segmented_step_bf16"] == S["grace_topk_segmented_step"]
    assert S["grace_topk_segmented_chunk_bf16"] == S["grace_topk_segmented_chunk"]


def test_segmented_chunk_lengths():
    """bf16: 20 float4 per lane with a residual stream, 32 without; f32 as it was."""
    from grace_amd import _lib
    bf16 = [int(_lib.query("grace_topk_segmented_chunk_bf16", r, d)) for r, d in CASES]
    f32 = [int(_lib.query("grace_topk_segmented_chunk", r, d)) for r, d in CASES]
    assert bf16 == [20480, 20480, 32768, 32768]
    assert f32 == [12288, 20480, 20480, 32768]


def test_segmented_bf16_argument_errors_do_not_touch_the_device():
    from grace_amd import _lib
    lib = _lib.load()
    nul = [None] * 3
    st = lib.grace_topk_segmented_step_bf16(None, None, 0, 1.0, 1.0, None, None, None, 0, None, 0, None, None, 0,
                                            None, None, None, 0, 0, *nul, None, None, 0, None, 0, 0, None)
    assert st == -1
    assert b"grace_topk_segmented_step_bf16" in lib.grace_last_error()
    st = lib.grace_topk_segmented_step(None, None, 0, 1.0, 1.0, None, None, None, 0, None, 0, None, None, 0,
                                       None, None, None, 0, 0, *nul, None, None, 0, None, 0, 0, None)
    assert st == -1
    assert b"grace_topk_segmented_step:" in lib.grace_last_error()
