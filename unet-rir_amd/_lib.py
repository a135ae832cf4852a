"""ctypes binding of libunetrir.so, derived from include/unetrir.h when this module is imported.

The header is the one place where the C ABI is written down: its function declarations become `FUNCS` (restype, argtypes and
parameter names), its `typedef struct`s the ctypes mirrors (ConvGeom, Config, CastDesc, ReduceDesc, LambSeg) and its integer
`#define UNETRIR_<NAME>`s `CONSTS`.  A new entry point is declared there and wrapped in ops.py; nothing is repeated here.

Type rule: a scalar (`_SCALARS`) is its ctypes twin; a pointer to a struct of the header is POINTER(mirror); every other pointer is
c_void_p, because device addresses travel as integers.  The parameters for which host and device differ from that rule are listed in
`_EXCEPTIONS`, by function and parameter name, and nowhere else.  Whatever the rule cannot map raises at import and names the offender.

There is no CPU fallback: if the library is missing or a call fails, this raises.
"""
import ctypes as C
import functools
import os
import re

from . import build as _build


class UnetrirError(RuntimeError):
    pass


_SCALARS = {"int": C.c_int, "long long": C.c_longlong, "unsigned long long": C.c_ulonglong, "float": C.c_float,
            "double": C.c_double, "size_t": C.c_size_t, "unetrir_stream_t": C.c_void_p}

_EXCEPTIONS = {                                                     # (function, parameter): host arrays, and device-resident structs
    **{("unetrir_stage_h2d", p): C.POINTER(C.c_void_p) for p in ("src", "pinned", "dev")},
    ("unetrir_stage_h2d", "bytes"): C.POINTER(C.c_size_t),
    **{(f"unetrir_spectral_loss{form}", "res"): C.POINTER(C.c_int)   # a host array of 3 R ints
       for form in ("_ws_bytes", "_f32", "_fft_ws_bytes", "_fft_f32")},
    ("unetrir_prof_collect", "counts"): C.POINTER(C.c_int),
    ("unetrir_prof_collect", "ms"): C.POINTER(C.c_double),
    ("unetrir_prof_collect", "flops"): C.POINTER(C.c_double),
    ("unetrir_lamb_f32", "segs"): C.c_void_p,                       # the table in device memory (segs_host follows the rule)
    ("unetrir_lamb_dev_f32", "segs"): C.c_void_p,
    ("unetrir_cast_weights_batched_bf16", "desc"): C.c_void_p,      # descriptors in device memory
    ("unetrir_resample_table_f32", "table"): C.POINTER(C.c_float),  # a host array of L T floats
}


_DECL = re.compile(r"([^,]*[\s*])(\w+(?:\s*,\s*\w+)*)", re.S)       # type, then a name (a struct field: or a comma list of names)


@functools.lru_cache(None)                                          # 1700 parameters, a few hundred distinct spellings
def _decl(text):
    """'const unetrir_bf16* const* w' -> ('unetrir_bf16', 2, ['w']): base type, pointer depth, names.  None: cannot be mapped."""
    m = _DECL.fullmatch(text)
    base, stars = (" ".join(re.sub(r"\bconst\b|\*", " ", m.group(1)).split()), m.group(1).count("*")) if m else ("", 0)
    return (base, stars, re.split(r"\s*,\s*", m.group(2))) if stars or base in _SCALARS else None


def parse_header(text, exceptions=None):
    """(funcs, structs, consts) of a header text: funcs[name] = (restype, [argtypes], [parameter names]); structs[C name] = a
    ctypes.Structure named in CamelCase without the prefix; consts[NAME] = int for every `#define UNETRIR_NAME <integer>`."""
    exceptions = dict(exceptions or {})
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    consts = {n: int(v, 0) for n, v in re.findall(r"^[ \t]*#[ \t]*define[ \t]+UNETRIR_(\w+)[ \t]+(-?(?:0[xX][0-9a-fA-F]+|\d+))[ \t]*$",
                                                  text, re.M)}
    structs = {}
    for m in re.finditer(r"\btypedef\s+struct\s*\w*\s*\{([^{}]*)\}\s*(unetrir_\w+)\s*;", text):
        fields = []
        for decl in filter(None, (d.strip() for d in m.group(1).split(";"))):
            d = _decl(decl)
            if d is None:
                raise UnetrirError(f"include/unetrir.h: struct {m.group(2)}: cannot map the field declaration '{decl}'")
            base, stars, names = d
            fields += [(n, C.c_void_p if stars else _SCALARS[base]) for n in names]
        py_name = "".join(w.capitalize() for w in m.group(2).split("_")[1:])
        structs[m.group(2)] = type(py_name, (C.Structure,), {"_fields_": fields, "__doc__": f"{m.group(2)} (include/unetrir.h)"})
    if len(structs) != len(re.findall(r"\btypedef\s+struct\b", text)):
        raise UnetrirError(f"include/unetrir.h: a typedef struct beside {sorted(structs)} did not parse")
    funcs = {}
    for m in re.finditer(r"^((?:\w+[ \t]+)+)(unetrir_\w+)\s*\(([^()]*)\)\s*;", text, re.M):
        ret, name, params = " ".join(m.group(1).split()), m.group(2), m.group(3).strip()
        if ret not in _SCALARS:
            raise UnetrirError(f"include/unetrir.h: {name}: cannot map the return type '{ret}'")
        argtypes, argnames = [], []
        for p in ([] if params in ("", "void") else params.split(",")):
            d = _decl(p.strip())
            if d is None:
                raise UnetrirError(f"include/unetrir.h: {name}: cannot map the parameter '{p.strip()}'")
            base, stars, (pname,) = d
            rule = C.POINTER(structs[base]) if stars == 1 and base in structs else C.c_void_p if stars else _SCALARS[base]
            argtypes.append(exceptions.pop((name, pname), rule))
            argnames.append(pname)
        funcs[name] = (_SCALARS[ret], argtypes, argnames)
    unparsed = sorted(set(re.findall(r"\b(unetrir_\w+)\s*\(", text)) - set(funcs))
    if unparsed:
        raise UnetrirError(f"include/unetrir.h: no binding could be derived for {unparsed}")
    if exceptions:
        raise UnetrirError(f"_lib._EXCEPTIONS names what include/unetrir.h does not declare: {sorted(exceptions)}")
    return funcs, structs, consts


with open(_build.HEADER) as _f:
    FUNCS, _STRUCTS, CONSTS = parse_header(_f.read(), _EXCEPTIONS)
ConvGeom, Config, CastDesc, ReduceDesc, LambSeg = (_STRUCTS["unetrir_" + n] for n in ("conv_geom", "config", "cast_desc", "reduce_desc",
                                                                                     "lamb_seg"))
EXPORTS = tuple(FUNCS)
ABI_VERSION, EINVAL, PROF_FAMILIES = CONSTS["ABI_VERSION"], CONSTS["EINVAL"], CONSTS["PROF_FAMILIES"]

_LIB = None
_LIB_PATH = None


def use_library(path):
    """Load another build of the library instead of libunetrir.so (scripts/: the timing-ablation build).  Before first use."""
    global _LIB_PATH
    if _LIB is not None:
        raise UnetrirError("the library is already loaded")
    _LIB_PATH = path


def bind(L, name):
    """Give export `name` of the loaded library L the header's restype and argtypes."""
    fn = getattr(L, name)      # AttributeError if the export is missing: fail loudly
    fn.restype, fn.argtypes = FUNCS[name][:2]
    return fn


def lib():
    """Load (building first if the sources are newer) libunetrir.so.  Raises if it cannot."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = _LIB_PATH or _build.LIB
    if _LIB_PATH is None and _build.needs_build():
        path = _build.build()
    if not os.path.exists(path):
        raise UnetrirError(f"HIP extension missing: {path}")
    L = C.CDLL(path)
    for name in EXPORTS:
        bind(L, name)
    if L.unetrir_abi_version() != ABI_VERSION:
        raise UnetrirError("libunetrir.so ABI version mismatch")
    _LIB = L
    return L


def check(err, what):
    if err != 0:
        raise UnetrirError(f"{what} failed with code {err}")
