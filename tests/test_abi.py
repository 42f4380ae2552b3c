"""The C ABI library loads without a GPU and exports every symbol include/grace_hip.h declares
(no compute calls here)."""
import ctypes
import os

import pytest

from tests.abi_util import HEADERS, check_types, declared, header


def declared_functions():
    return declared(header("grace_hip.h"))


def test_header_declares_functions():
    names = declared_functions()
    assert "grace_topk_residual_step" in names and len(names) >= 20


def test_library_exports_every_declared_symbol():
    from grace_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail(f"native library not built: {_lib.LIB_PATH}")
    lib = ctypes.CDLL(_lib.LIB_PATH)
    missing = [n for n in declared_functions() if not hasattr(lib, n)]
    assert not missing, missing


def test_binding_table_matches_header():
    from grace_amd import _lib
    assert sorted(_lib.SIGNATURES) == declared_functions()


@pytest.mark.parametrize("name,table", zip(HEADERS, ("SIGNATURES", "SIGNATURES_SIGN", "SIGNATURES_QUANT",
                                                     "SIGNATURES_DGC", "SIGNATURES_SPARSE")))
def test_binding_table_types_match_prototypes(name, table):
    """All 191 entries, by a reading of the prototypes that is not the binding's own parser."""
    from grace_amd import _lib
    hdr = header(name)
    assert sorted(getattr(_lib, table)) == declared(hdr)
    check_types(hdr, getattr(_lib, table))


def test_version_and_error_channel():
    from grace_amd import _lib
    lib = _lib.load()
    assert lib.grace_version() >= 100
    # an argument error is reported without touching the device
    st = lib.grace_axpby(None, None, 1.0, 1.0, None, 10, None)
    assert st == -1
    assert b"grace_axpby" in lib.grace_last_error()


def test_product_path_refuses_cpu_tensors():
    import torch
    from grace_amd.dist.compressor.topk import TopKCompressor
    from grace_amd.ops import GraceDeviceError
    with pytest.raises(GraceDeviceError):
        TopKCompressor(0.01).compress(torch.randn(100), "w")
