"""grace_amd._lib.parse_header on synthetic header text (every type, every layout it has to read,
every case in which it must refuse) and, spelled out by hand, what it makes of ten awkward real entry
points.  No GPU and no library: only the module's import, which reads the five headers."""
from ctypes import c_char_p, c_double, c_float, c_int, c_int32, c_int64, c_size_t, c_uint16, c_uint32, c_uint64
from ctypes import c_void_p as P

import pytest

from grace_amd import _lib
from grace_amd._lib import GraceNativeError, parse_header

SCALARS = {"float": c_float, "double": c_double, "int": c_int, "int32_t": c_int32, "int64_t": c_int64,
           "uint16_t": c_uint16, "uint32_t": c_uint32, "uint64_t": c_uint64, "size_t": c_size_t,
           "grace_status_t": c_int}


def same(got, want):
    """The same names in the same order, every restype and argtype the same ctypes object."""
    assert list(got) == list(want)
    for name, (res, args) in want.items():
        assert got[name][0] is res, name
        assert len(got[name][1]) == len(args) and all(a is b for a, b in zip(got[name][1], args)), name


@pytest.mark.parametrize("word", sorted(SCALARS))
def test_every_scalar_type_as_parameter_and_result(word):
    got = parse_header(f"{word} grace_a({word} x);\ngrace_status_t grace_b(const {word} y, {word});", "t.h")
    same(got, {"grace_a": (SCALARS[word], [SCALARS[word]]), "grace_b": (c_int, [SCALARS[word], SCALARS[word]])})


def test_pointers_however_they_are_spelled():
    got = parse_header("grace_status_t grace_p(const float* a, float *b, uint16_t* c, void** d, const void *e,\n"
                       "                       unknown_t* f, int64_t n);", "t.h")
    same(got, {"grace_p": (c_int, [P, P, P, P, P, P, c_int64])})


def test_empty_parameter_lists_and_results():
    got = parse_header("int grace_v(void);\nconst char* grace_e();\nsize_t grace_s( void );\n"
                       "const char *grace_f(void);\nint32_t grace_g( );", "t.h")
    same(got, {"grace_v": (c_int, []), "grace_e": (c_char_p, []), "grace_s": (c_size_t, []),
               "grace_f": (c_char_p, []), "grace_g": (c_int32, [])})


def test_a_prototype_over_three_lines_and_comments_that_name_calls():
    text = """
/* as grace_x( in a block comment, over
 * two lines: grace_y(int a); */
#ifdef __cplusplus
extern "C" {
#endif
typedef int grace_status_t;
// a line comment: grace_z(float q);
grace_status_t grace_long(const float* g, int64_t n,   /* trailing grace_w( */
                          double ratio,
                          size_t ws_bytes, void* stream);   // and grace_u(
size_t grace_bytes(int64_t n);
#ifdef __cplusplus
}
#endif
"""
    same(parse_header(text, "t.h"), {"grace_long": (c_int, [P, c_int64, c_double, c_size_t, P]),
                                     "grace_bytes": (c_size_t, [c_int64])})


@pytest.mark.parametrize("text,symbol", [
    ("grace_status_t grace_a(int8_t x);", "grace_a"),                     # a scalar type it does not know
    ("grace_status_t grace_a(unsigned int x);", "grace_a"),
    ("grace_status_t grace_a(float x[4]);", "grace_a"),
    ("grace_status_t grace_a(int64_t n, ...);", "grace_a"),
    ("bool grace_a(void);", "grace_a"),                                   # ... as the result
    ("void grace_a(int x);", "grace_a"),
    ("unsigned int grace_a(void);", "grace_a"),                           # the result is read whole
    ("long int grace_a(void);", "grace_a"),
    ("short int grace_a(int x);", "grace_a"),
    ("const int grace_a(void);", "grace_a"),
    ("int grace_ok(void);\nunsigned\nint grace_a(void);", "grace_a"),
    ("extern int grace_a(void);", "grace_a"),
    ("char* grace_a(void);", "grace_a"),                                  # only `const char*` is a string
    ("grace_a(void);", "grace_a"),
    ("int grace_ok(void);\n#if 0\nint grace_a(void);\n#endif", "#if 0"),   # a conditional could hide one
    ("#ifdef GRACE_EXTRA\nint grace_a(void);\n#endif", "#ifdef GRACE_EXTRA"),
    ("#ifdef __cplusplus\n#else\nint grace_a(void);\n#endif", "#else"),
    ("#define grace_m(x) (x)\nint grace_ok(void);", "grace_m"),
    ("int grace_ok(void);\nint grace_cb(void (*f)(int));", "grace_cb"),  # a grace_...( the pattern did not consume
    ("int grace_ok(void);\n#define grace_m(x) (x)", "grace_m"),
    ("static inline int grace_i(int x) { return x; }", "grace_i"),
    ("int grace_ok(void);\nint grace_open(int x", "grace_open"),
    ("int grace_a(void);\nint grace_b(int x);\nint grace_a(void);", "grace_a"),   # declared twice
])
def test_fails_closed_naming_header_and_symbol(text, symbol):
    with pytest.raises(GraceNativeError) as e:
        parse_header(text, "grace_t.h")
    assert "grace_t.h" in str(e.value) and symbol in str(e.value)


def test_names_in_any_case_and_prototypes_on_one_line():
    got = parse_header("int grace_A(int x);int grace_b2(void); size_t grace_c(void);", "t.h")
    same(got, {"grace_A": (c_int, [c_int]), "grace_b2": (c_int, []), "grace_c": (c_size_t, [])})


def test_a_name_declared_in_two_headers():
    seen = {}
    parse_header("int grace_a(void);", "one.h", seen)
    parse_header("int grace_b(void);", "two.h", seen)
    assert seen == {"grace_a": "one.h", "grace_b": "two.h"}
    with pytest.raises(GraceNativeError) as e:
        parse_header("int grace_c(void);\nint grace_a(int x);", "three.h", seen)
    assert "three.h" in str(e.value) and "grace_a" in str(e.value) and "one.h" in str(e.value)


def test_a_header_that_cannot_be_read():
    with pytest.raises(GraceNativeError) as e:
        _lib._header_table("grace_hip_missing.h")
    assert "grace_hip_missing.h" in str(e.value)


def test_the_real_tables_name_nothing_twice():
    tables = (_lib.SIGNATURES, _lib.SIGNATURES_SIGN, _lib.SIGNATURES_QUANT, _lib.SIGNATURES_DGC,
              _lib.SIGNATURES_SPARSE)
    assert sum(len(t) for t in tables) == len(set().union(*tables)) == 191
    names = (_lib.P, _lib.I32, _lib.I64, _lib.F32, _lib.U64, _lib.SZ, _lib.ST)
    assert names == (P, c_int32, c_int64, c_float, c_uint64, c_size_t, c_int)


I32, I64, F32, U64, SZ, ST = c_int32, c_int64, c_float, c_uint64, c_size_t, c_int
# read off the prototypes by hand
REAL = {
    "grace_version": ("SIGNATURES", c_int, []),
    "grace_last_error": ("SIGNATURES", c_char_p, []),
    "grace_fill_bf16": ("SIGNATURES", ST, [P, c_uint16, I64, P]),
    "grace_dgc_threshold": ("SIGNATURES", ST, [P, I64, P, I64, c_double, P, P]),
    "grace_topk_main_grid_limit": ("SIGNATURES", c_uint32, [c_uint32]),
    "grace_qsgd_global_compress": ("SIGNATURES", ST, [P, I64, I32, P, U64, P, P, P, P, P]),
    "grace_topk_segmented_step_bf16": ("SIGNATURES", ST, [P, P, I32, F32, F32, P, P, P, I32, P, I32, P, P, I64, P, P, P,
                                                         I64, I64, P, P, P, P, P, I32, P, SZ, I64, P]),
    "grace_efsign_workspace_bytes": ("SIGNATURES_SIGN", SZ, [I64]),
    "grace_dgc_sample_kth_workspace_bytes": ("SIGNATURES", SZ, []),
    "grace_sparse_aggregate_padded_bf16": ("SIGNATURES_SPARSE", ST, [P, I64, P, I32, F32, P, I64, P, SZ, P]),
}


@pytest.mark.parametrize("name", sorted(REAL))
def test_real_entry_point(name):
    table, res, args = REAL[name]
    got = getattr(_lib, table)[name]
    assert got[0] is res
    assert len(got[1]) == len(args) and all(a is b for a, b in zip(got[1], args)), got[1]
