"""What the tests/test_abi*.py files share: the headers under include/ read as text, a type check of
the binding tables that does not go through grace_amd._lib's own parser, and the stand-ins that let the
Python wrappers be driven as far as their own checks without a GPU."""
import ctypes
import inspect
import os
import re
import textwrap

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADERS = ("grace_hip.h", "grace_hip_sign.h", "grace_hip_quant.h", "grace_hip_dgc.h", "grace_hip_sparse.h")
# the scalar types of the C ABI, spelled out here a second time on purpose (grace_status_t is an int)
CTYPE_OF = {"float": ctypes.c_float, "double": ctypes.c_double, "int": ctypes.c_int, "int32_t": ctypes.c_int32,
            "int64_t": ctypes.c_int64, "uint16_t": ctypes.c_uint16, "uint32_t": ctypes.c_uint32,
            "uint64_t": ctypes.c_uint64, "size_t": ctypes.c_size_t, "grace_status_t": ctypes.c_int}


def header(name):
    hdr = open(os.path.join(ROOT, "include", name)).read()
    return re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)


def declared(hdr):
    return sorted(set(re.findall(r"\b(grace_[a-z0-9_]+)\s*\(", hdr)))


def params(hdr, name):
    m = re.search(r"\b%s\s*\(([^)]*)\)" % name, hdr)
    assert m, f"{name} is not declared"
    return re.sub(r"\s+", " ", m.group(1)).strip()


def check_types(hdr, table):
    """Every entry of a binding table against its prototype in `hdr`: as many arguments, a `*` means
    a pointer, anything else is looked up by its type token; the result is what stands in front of
    the name on its line.  Deliberately not grace_amd._lib's parser: the tables are derived from the
    headers, and this is what keeps them from being compared with themselves."""
    for name, (res, args) in table.items():
        ps = params(hdr, name)
        ps = [] if ps in ("", "void") else [p.strip() for p in ps.split(",")]
        assert len(args) == len(ps), name
        for p, a in zip(ps, args):      # each bound type is the prototype's
            want = ctypes.c_void_p if "*" in p else CTYPE_OF[p.rsplit(" ", 1)[0]]
            assert a is want, (name, p)
        ret = re.search(r"^(.*?)\b%s\s*\(" % name, hdr, flags=re.M).group(1).strip()
        assert res is (ctypes.c_char_p if "*" in ret else CTYPE_OF[ret]), (name, ret)


def check_bad(lib, name, good, bad):
    f = getattr(lib, name)
    for i, v in bad:
        args = list(good)
        args[i] = v
        assert f(*args) == -1, (name, i, v)
        assert lib.grace_last_error().startswith(name.encode() + b":"), lib.grace_last_error()


class OnGpu(torch.Tensor):
    """A CPU tensor that says it is on the GPU, so that the wrappers get as far as their own checks."""
    device = property(lambda self: torch.device("cuda", 0))
    is_cuda = property(lambda self: True)


def no_native(monkeypatch):
    from grace_amd import _lib

    def no_native(*a, **kw):
        raise AssertionError("a native call was made")
    for attr in ("call", "query", "fn", "load"):
        monkeypatch.setattr(_lib, attr, no_native)


def body(fn):
    src = textwrap.dedent(inspect.getsource(fn))
    src = re.sub(r'""".*?"""', "", src, count=1, flags=re.S)     # the docstring
    return [ln.rstrip() for ln in src.split("\n")[1:] if ln.strip()]  # without the def line
