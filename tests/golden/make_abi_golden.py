"""Generates tests/golden/abi_v1.json: the ctypes binding of ABI version 1 as the loaded library carries it - recorded while
unet_rir_amd/_lib.py still held the table by hand, so that tests/test_abi_table.py can hold the binding derived from include/unetrir.h
to it.  Strings and integers only: exact, and the same on every machine.

Everything is read back from bound objects, never from a source text, so the script gives the same file whichever way the binding
was made:
    functions  per name of _lib.EXPORTS, [restype, [argtypes...]] of the function object of _lib.lib(), as ctypes type names with
               POINTER(X) spelled out
    structs    per mirror (ConvGeom, Config, CastDesc, ReduceDesc, LambSeg) its _fields_ as [name, type name], its sizeof and the
               offset of every field
    constants  the eight integers of the header: ABI_VERSION and EINVAL as the library answers them (unetrir_abi_version(), and
               a reduction of one descriptor without a descriptor array), the others as _lib and ops carry them

    python tests/golden/make_abi_golden.py [output file]
"""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:          # run as a script (under pytest, tests/conftest.py has put ROOT there)
    sys.path.insert(0, ROOT)

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "abi_v1.json")
STRUCTS = ("ConvGeom", "Config", "CastDesc", "ReduceDesc", "LambSeg")


def type_name(t):
    if t is None:
        return "None"
    if issubclass(t, C._Pointer):
        return f"POINTER({type_name(t._type_)})"
    return t.__name__


def record():
    import unet_rir_amd as U
    _lib, ops = U._lib, U.ops
    L = _lib.lib()
    functions = {}
    for name in _lib.EXPORTS:
        fn = getattr(L, name)
        functions[name] = [type_name(fn.restype), [type_name(a) for a in fn.argtypes]]
    structs = {}
    for s in STRUCTS:
        cls = getattr(_lib, s)
        structs[s] = {"fields": [[n, type_name(t)] for n, t in cls._fields_], "sizeof": C.sizeof(cls),
                      "offsets": {n: getattr(cls, n).offset for n, _ in cls._fields_}}
    constants = {"ABI_VERSION": L.unetrir_abi_version(), "EINVAL": L.unetrir_splitk_reduce_batched(None, 1, None),
                 "PROF_FAMILIES": _lib.PROF_FAMILIES, "LAMB_DECAY": ops.LAMB_DECAY, "LAMB_ADAPT": ops.LAMB_ADAPT,
                 "C22_FWD": ops.C22_FWD, "C22_DGRAD": ops.C22_DGRAD, "C22_WGRAD": ops.C22_WGRAD}
    return {"constants": constants, "structs": structs, "functions": functions}


def dumps(rec):
    """One line per function and per struct, names sorted: the order of the table does not reach the file."""
    def block(d):
        return "{\n" + ",\n".join(f"  {json.dumps(k)}: {json.dumps(d[k], sort_keys=True)}" for k in sorted(d)) + "\n }"
    return ("{\n" + f' "constants": {json.dumps(rec["constants"], sort_keys=True)},\n' + f' "structs": {block(rec["structs"])},\n'
            + f' "functions": {block(rec["functions"])}\n' + "}\n")


if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else OUT
    with open(out, "w") as f:
        f.write(dumps(record()))
    print(out)
