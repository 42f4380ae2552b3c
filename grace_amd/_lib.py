"""ctypes binding of libgrace_hip.so (the C ABI declared in include/grace_hip.h,
include/grace_hip_sign.h, include/grace_hip_quant.h, include/grace_hip_dgc.h,
include/grace_hip_sparse.h and include/grace_hip_cast.h).

The headers are the declaration: the binding tables below are parsed from their prototypes at
import.  A new entry point is declared in its header and defined in the .hip that includes that
header; nothing is typed a second time here.  A prototype the parser does not fully understand
raises at import: no type is ever guessed.

The library is the only compute path of grace_amd: there is no CPU or eager-PyTorch fallback.
If the shared object is missing (not built) or a tensor is not on the GPU, calls raise.
"""
import ctypes
import os
import re
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("GRACE_HIP_LIB", os.path.join(_HERE, "lib", "libgrace_hip.so"))
INCLUDE_DIR = os.path.join(os.path.dirname(_HERE), "include")

P = ctypes.c_void_p
I32 = ctypes.c_int32
I64 = ctypes.c_int64
F32 = ctypes.c_float
U64 = ctypes.c_uint64
SZ = ctypes.c_size_t
ST = ctypes.c_int


class GraceNativeError(RuntimeError):
    """A native call failed or the native library is unavailable."""


# the scalar types of the C ABI; a parameter with a `*` is an address (P), whatever it points to
_SCALARS = {"float": F32, "double": ctypes.c_double, "int": ctypes.c_int, "int32_t": I32, "int64_t": I64,
            "uint16_t": ctypes.c_uint16, "uint32_t": ctypes.c_uint32, "uint64_t": U64, "size_t": SZ,
            "grace_status_t": ST}
_COMMENT = re.compile(r"/\*.*?\*/|//[^\n]*", re.S)
# the only conditionals understood: the include guard and the `extern "C"` guard, which hide nothing
_CONDITIONAL = re.compile(r"^[ \t]*#[ \t]*(?:if|ifdef|ifndef|elif|else)\b"
                          r"(?![ \t]+(?:__cplusplus|GRACE_HIP\w*_H)\b)[^\n]*", re.M)
_NAME = re.compile(r"\b(grace_\w+)\s*\(")
# what precedes the declaration (the start, `;`, `{`, `}` or a preprocessor line), everything between
# that and the name (the result's type, whole), the name, the parameter list; the closing `;` stays
_PROTO = re.compile(r"(\A|[;{}]|(?m:^[ \t]*#[^\n]*\n))\s*([^;{}#()]*?)\b(grace_\w+)\s*\(([^()]*)\)\s*(?=;)")
_SCALAR_PARAM = re.compile(r"\s*(?:const\s+)?(\w+)(?:\s+\w+)?\s*")


def _scalar(word, header, name, what):
    if word not in _SCALARS:
        raise GraceNativeError(f"{header}: {name}: {what} has a type the binding does not know")
    return _SCALARS[word]


def parse_header(text, header, seen=None):
    """{name: (restype, [argtypes])} of the prototypes in the header text `text`, in declaration order;
    `header` names the text in errors.  `seen` (name -> header, updated) spans several headers: a name
    declared twice raises, and so do a result that is neither `const char*` nor one word of _SCALARS,
    a scalar parameter outside _SCALARS, a `grace_...(` that is not part of a prototype this parser
    understands, and a preprocessor conditional other than the two guards (it could hide a prototype)."""
    seen = {} if seen is None else seen
    text = _COMMENT.sub(" ", text)
    cond = _CONDITIONAL.search(text)
    if cond:
        raise GraceNativeError(f"{header}: the binding does not evaluate `{cond.group().strip()}`")
    table = {}
    for _, ret, name, params in _PROTO.findall(text):
        if name in seen:
            raise GraceNativeError(f"{header}: {name} is already declared in {seen[name]}")
        seen[name] = header
        ret = re.sub(r"\s*\*\s*", "*", " ".join(ret.split()))
        res = ctypes.c_char_p if ret == "const char*" else _scalar(ret, header, name, f"the result `{ret}`")
        args = []
        for p in (params.split(",") if params.strip() not in ("", "void") else ()):
            m = _SCALAR_PARAM.fullmatch(p)
            args.append(P if "*" in p else _scalar(m and m.group(1), header, name, f"parameter `{p.strip()}`"))
        table[name] = (res, args)
    left = _NAME.search(_PROTO.sub(r"\1 ", text))
    if left:
        raise GraceNativeError(f"{header}: {left.group(1)}( is not in a prototype the binding can parse")
    return table


_declared = {}


def _header_table(header):
    """The binding table of include/<header>, read when this module is imported."""
    try:
        with open(os.path.join(INCLUDE_DIR, header)) as f:
            text = f.read()
    except OSError as e:
        raise GraceNativeError(f"{header}: cannot read the header the binding is derived from ({e})") from e
    return parse_header(text, header, _declared)


# name -> (restype, argtypes): one table a header, every prototype of that header
SIGNATURES = _header_table("grace_hip.h")
# the sign family on bfloat16 and the fused EF-signSGD step
SIGNATURES_SIGN = _header_table("grace_hip_sign.h")
# QSGD and TernGrad on bfloat16
SIGNATURES_QUANT = _header_table("grace_hip_quant.h")
# DGC on bfloat16; the records decode with a bf16 dense result
SIGNATURES_DGC = _header_table("grace_hip_dgc.h")
# threshold and random-k on bfloat16; the padded decode with a bf16 dense result
SIGNATURES_SPARSE = _header_table("grace_hip_sparse.h")
# natural, cnat, fp16 and one-bit on bfloat16; one-bit's fused step and W-rank decode
SIGNATURES_CAST = _header_table("grace_hip_cast.h")

_lock = threading.Lock()
_lib = None
_handles = {}
_fns = {}


def _bind(lib, strict):
    """Give every symbol of the six tables its restype and argtypes and return `lib`.  strict: a
    symbol the library lacks raises AttributeError; otherwise it stays unbound."""
    for name, (res, args) in (*SIGNATURES.items(), *SIGNATURES_SIGN.items(), *SIGNATURES_QUANT.items(),
                              *SIGNATURES_DGC.items(), *SIGNATURES_SPARSE.items(), *SIGNATURES_CAST.items()):
        f = getattr(lib, name) if strict else getattr(lib, name, None)
        if f is not None:
            f.restype = res
            f.argtypes = args
    return lib


def load():
    """Load (once) and return the ctypes handle; raises GraceNativeError if it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is None:
            if not os.path.exists(LIB_PATH):
                raise GraceNativeError(
                    f"grace_amd native library not found at {LIB_PATH}; build it with "
                    "`python -c 'import __graft_entry__ as g; g.build()'` (no CPU fallback exists)")
            _lib = _bind(ctypes.CDLL(LIB_PATH), strict=True)
    return _lib


def use(path):
    """Make the build of the library at `path` the one every later call goes to, and return its
    handle (tools that A/B two builds in one process).  An older build may lack newer symbols: those
    stay unbound and raise AttributeError only if called."""
    global _lib
    with _lock:
        lib = _handles.get(path)
        if lib is None:
            lib = _handles[path] = _bind(ctypes.CDLL(os.path.abspath(path)), strict=False)
        _lib = lib
        _fns.clear()
    return lib


def fn(name):
    """The resolved ctypes function (for launch-bound callers that check the status themselves)."""
    f = _fns.get(name)
    if f is None:   # first use: resolve once (the per-call CDLL attribute lookup costs host time
        f = _fns[name] = getattr(load(), name)   # on launch-bound steps such as a 4 MiB sign step)
    return f


def _fail(name, st):
    msg = load().grace_last_error()
    raise GraceNativeError(f"{name} failed ({st}): {msg.decode() if msg else ''}")


def call(name, *args):
    f = _fns.get(name)
    if f is None:
        f = fn(name)
    st = f(*args)
    if st != 0:
        _fail(name, st)
    return st


def check(name, st):
    if st != 0:
        _fail(name, st)


def query(name, *args):
    return fn(name)(*args)
