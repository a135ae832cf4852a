"""The ctypes binding that unet_rir_amd/_lib.py derives from include/unetrir.h, checked without a GPU.

THE RULE OF THE ABI VERSION.  tests/golden/abi_v1.json (tests/golden/make_abi_golden.py) records every function, struct and constant of
ABI version 1 as the binding carried them when the table was still written by hand.  While UNETRIR_ABI_VERSION is 1, a pull request
may ADD functions, structs and constants that the file lacks; it may not change the return type, an argument type, the argument count,
a struct's fields, layout or size, or a constant's value of a recorded one.  Changing a recorded entry means a new ABI version and a new
file beside this one.

The struct layouts are held to the C compiler, the parser to small synthetic headers: its edge cases, and every input it must refuse."""
import ctypes as C
import importlib.util
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def lib_mod():
    import unet_rir_amd
    return unet_rir_amd._lib


@pytest.fixture(scope="module")
def bound():
    """What the recorder reads back from the binding of this tree."""
    spec = importlib.util.spec_from_file_location("make_abi_golden", os.path.join(GOLDEN, "make_abi_golden.py"))
    rec = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rec)
    return rec.record()


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(GOLDEN, "abi_v1.json")) as f:
        return json.load(f)


def test_recorded_abi_v1_is_unchanged(lib_mod, bound, recorded):
    """Every recorded entry is in the derived binding with identical types, layout and value (additions are free: see the rule above)."""
    assert lib_mod.ABI_VERSION == 1 == recorded["constants"]["ABI_VERSION"]
    assert len(recorded["functions"]) == 197 and len(recorded["structs"]) == 5 and len(recorded["constants"]) == 8
    for name, sig in recorded["functions"].items():
        assert bound["functions"].get(name) == sig, name
    for name, layout in recorded["structs"].items():
        assert bound["structs"].get(name) == layout, name
    for name, value in recorded["constants"].items():
        assert bound["constants"].get(name) == value, name
        assert lib_mod.CONSTS[name] == value, name                # the header's own #define, not only what the library answers
    assert lib_mod.EINVAL == 10001 and lib_mod.PROF_FAMILIES == 8


def test_table_is_the_header(lib_mod):
    assert lib_mod.EXPORTS == tuple(lib_mod.FUNCS)
    for name, (_, argtypes, argnames) in lib_mod.FUNCS.items():
        assert len(argtypes) == len(argnames) == len(set(argnames)), name
    for (fn, param), t in lib_mod._EXCEPTIONS.items():
        assert lib_mod.FUNCS[fn][1][lib_mod.FUNCS[fn][2].index(param)] is t, (fn, param)


def _host_clang():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")          # what build.py compiles the library with
    here = os.path.dirname(os.path.realpath(shutil.which(hipcc) or hipcc))
    for c in (os.path.join(here, "amdclang"), os.path.join(here, "..", "lib", "llvm", "bin", "clang")):
        if os.path.exists(c):
            return c
    raise AssertionError(f"no clang beside {hipcc}")


def test_struct_layouts_match_the_compiler(lib_mod, tmp_path):
    """The header compiles as strict C99, and the compiler's sizeof / offsetof of every field equal the ctypes mirrors'."""
    import unet_rir_amd
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "unetrir.h"', 'int main(void) {']
    want = []
    for cname, cls in lib_mod._STRUCTS.items():
        lines.append(f'    printf("{cname} %lu\\n", (unsigned long)sizeof({cname}));')
        want.append(f"{cname} {C.sizeof(cls)}")
        for field, _ in cls._fields_:
            lines.append(f'    printf("{cname}.{field} %lu %lu\\n", (unsigned long)offsetof({cname}, {field}), '
                         f'(unsigned long)sizeof((({cname}*)0)->{field}));')
            want.append(f"{cname}.{field} {getattr(cls, field).offset} {getattr(cls, field).size}")
    lines += ['    return 0;', '}']
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    subprocess.run([_host_clang(), "-x", "c", "-std=c99", "-Wall", "-Werror", "-pedantic",
                    "-I", os.path.dirname(unet_rir_amd.build.HEADER), str(src), "-o", str(exe)], check=True)
    got = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(lib_mod._STRUCTS) == 5 and got == want


SYNTHETIC = """
#ifndef UNETRIR_H
#define UNETRIR_H
#define UNETRIR_ANSWER 42
#define UNETRIR_MASK 0x10
typedef void* unetrir_stream_t;
typedef struct { int B, H, W; float* p; size_t n; } unetrir_anon;
typedef struct unetrir_tagged {
    long long a;         /* a comment; with a semicolon */
    const unetrir_bf16* q;
} unetrir_tagged;
int unetrir_zero(void);
/* between two declarations: int unetrir_ghost(int a); and a lone ) and ( */
long long unetrir_three(const unetrir_anon* g,      // a line comment (with parentheses);
                        unsigned long long seed, long long n,
                        const float* x, void** out, unetrir_stream_t stream);
size_t unetrir_after(const unetrir_tagged* t, double d, const void* const* list);
enum { UNETRIR_FAM_A = 0, UNETRIR_FAM_B = 1 };
#endif
"""


def test_parser_edge_cases(lib_mod):
    funcs, structs, consts = lib_mod.parse_header(SYNTHETIC, {("unetrir_three", "out"): C.POINTER(C.c_void_p)})
    assert consts == {"ANSWER": 42, "MASK": 16}
    anon, tagged = structs["unetrir_anon"], structs["unetrir_tagged"]
    assert list(structs) == ["unetrir_anon", "unetrir_tagged"] and (anon.__name__, tagged.__name__) == ("Anon", "Tagged")
    assert anon._fields_ == [("B", C.c_int), ("H", C.c_int), ("W", C.c_int), ("p", C.c_void_p), ("n", C.c_size_t)]
    assert tagged._fields_ == [("a", C.c_longlong), ("q", C.c_void_p)]
    assert list(funcs) == ["unetrir_zero", "unetrir_three", "unetrir_after"]
    assert funcs["unetrir_zero"] == (C.c_int, [], [])
    assert funcs["unetrir_three"] == (C.c_longlong, [C.POINTER(anon), C.c_ulonglong, C.c_longlong, C.c_void_p, C.POINTER(C.c_void_p),
                                                     C.c_void_p], ["g", "seed", "n", "x", "out", "stream"])
    assert funcs["unetrir_after"] == (C.c_size_t, [C.POINTER(tagged), C.c_double, C.c_void_p], ["t", "d", "list"])
    assert lib_mod.parse_header(SYNTHETIC)[0]["unetrir_three"][1][4] is C.c_void_p          # T** without an exception: the rule


@pytest.mark.parametrize("header, exceptions, offenders", [
    ("int unetrir_f(short s);", {}, ["unetrir_f", "short s"]),                                  # an unknown scalar type
    ("int unetrir_f(int);", {}, ["unetrir_f", "'int'"]),                                        # a parameter without a name
    ("short unetrir_f(int a);", {}, ["unetrir_f", "short"]),                                    # an unknown return type
    ("float* unetrir_f(int a);", {}, ["unetrir_f"]),                                            # a pointer return type
    ("int unetrir_ok(void);\nint unetrir_f(int (*cb)(int), int n);", {}, ["unetrir_f"]),        # a function-pointer parameter
    ("int unetrir_f(int n, ...);", {}, ["unetrir_f", "..."]),                                   # a variadic
    ("    int unetrir_f(int n);", {}, ["unetrir_f"]),                                           # not in column 0
    ("typedef struct { short s; } unetrir_bad;", {}, ["unetrir_bad", "short s"]),               # a struct field of an unknown type
    ("typedef struct { int *a, *b; } unetrir_bad;", {}, ["unetrir_bad", "int *a, *b"]),
    ("typedef struct { struct { int a; } in; } unetrir_bad;", {}, ["typedef struct"]),          # a struct the pattern does not take
    ("int unetrir_f(int n);", {("unetrir_f", "m"): C.c_void_p}, ["unetrir_f", "'m'"]),          # stale exception keys
    ("int unetrir_f(int n);", {("unetrir_g", "n"): C.c_void_p}, ["unetrir_g"]),
])
def test_parser_refuses_and_names_the_offender(lib_mod, header, exceptions, offenders):
    with pytest.raises(lib_mod.UnetrirError) as e:
        lib_mod.parse_header(header, exceptions)
    for o in offenders:
        assert o in str(e.value), (o, str(e.value))
