"""The bfloat16 top-k entry points are declared in include/grace_hip.h, exported by the library
and bound in grace_amd/_lib.py, and refuse bad arguments without touching the device (no GPU)."""
import ctypes
import re

import pytest

from tests.abi_util import header

NAMES = ["grace_topk_compress_bf16", "grace_topk_step_dense_bf16", "grace_topk_residual_step_bf16",
         "grace_topk_residual_step_swap_bf16", "grace_f32_to_bf16"]


@pytest.mark.parametrize("name", NAMES)
def test_bf16_entry_point_declared_exported_bound(name):
    from grace_amd import _lib
    hdr = header("grace_hip.h")
    assert re.search(r"\b%s\s*\(" % name, hdr), "not declared in include/grace_hip.h"
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name), "not exported by the library"
    assert name in _lib.SIGNATURES, "not bound in grace_amd/_lib.py"


def test_bf16_twins_mirror_f32_signatures():
    """g / x / out change type only (all pointers in the binding); the recycling parameters
    (prev_idx, prev_count) are dropped."""
    from grace_amd._lib import SIGNATURES as S
    assert S["grace_topk_compress_bf16"] == S["grace_topk_compress"]
    dense = list(S["grace_topk_step_dense"][1])
    assert S["grace_topk_step_dense_bf16"][1] == dense[:6] + dense[8:]
    carry = list(S["grace_topk_residual_step_carry"][1])
    assert S["grace_topk_residual_step_bf16"][1] == carry[:13] + carry[15:]
    assert S["grace_topk_residual_step_swap_bf16"] == S["grace_topk_residual_step_swap"]


def test_bf16_argument_errors_do_not_touch_the_device():
    from grace_amd import _lib
    lib = _lib.load()
    st = lib.grace_topk_compress_bf16(None, 10, 1, None, None, None, 0, None)
    assert st == -1
    assert b"grace_topk_compress_bf16" in lib.grace_last_error()
    st = lib.grace_f32_to_bf16(None, None, 10, None)
    assert st == -1
    assert b"grace_f32_to_bf16" in lib.grace_last_error()
    # a non-null gradient but a bad size is an argument error as well (nothing is launched)
    buf = (ctypes.c_uint16 * 4)()
    st = lib.grace_topk_residual_step_swap_bf16(ctypes.addressof(buf), None, 0, 1.0, 1.0, 0, 1, None, None, None,
                                                None, 0, 0, None, 0, None)
    assert st == -1
    assert b"grace_topk_residual_step_swap_bf16" in lib.grace_last_error()
