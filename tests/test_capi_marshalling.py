"""The Python binding without a GPU and without the library: what every wrapper of _capi.py hands to C and hands back
(tests/capi_trace.py drives the binding through a recording stand-in for libalmpc.so)."""
import ctypes
import difflib

import capi_trace


def test_binding_makes_the_recorded_calls(pkg):
    """Every public function and every Solver / Group method, with every optional-argument branch, makes the C calls of
    tests/golden/capi_calls.txt -- symbol, scalars, dtype and byte count of every buffer, the bytes of every const one -- and
    returns arrays of the recorded dtype, shape, strides and content."""
    got = capi_trace.trace(pkg._capi)
    want = open(capi_trace.GOLDEN).read().splitlines()
    diff = list(difflib.unified_diff(want, got, "tests/golden/capi_calls.txt", "the binding in the tree", lineterm="", n=2))
    assert not diff, "\n".join(diff[:80])


# functions of include/almpc.h the binding leaves out on purpose (none today: even the test hook almpc_debug_poison_lds has a wrapper)
NOT_BOUND = ()


def _class_of(ctype):
    """double / int / uint32 / pointer: what has to agree between a parameter of the header and its ctypes type"""
    if ctype is ctypes.c_double:
        return "double"
    if ctype in (ctypes.c_int, ctypes.c_int32):
        return "int"
    if ctype is ctypes.c_uint32:
        return "uint32"
    if ctype in (ctypes.c_void_p, ctypes.c_char_p) or issubclass(ctype, ctypes._Pointer):
        return "pointer"
    return repr(ctype)


def _class_of_c(ctype):
    if "*" in ctype:
        return "pointer"
    return {"double": "double", "int": "int", "int32_t": "int", "uint32_t": "uint32"}.get(ctype, ctype)


def test_prototype_table_agrees_with_the_header(pkg):
    """Every symbol of _capi.py's prototype table is declared by include/almpc.h with as many parameters, each of the same class
    (double, int, uint32_t, pointer), and the return types the table names are the header's; every declared function is in the
    table or in NOT_BOUND."""
    capi = pkg._capi
    declared, table = capi_trace.declarations(), capi.prototypes()
    wrong = []
    for name, argtypes in sorted(table.items()):
        if name not in declared:
            wrong.append(f"{name}: not declared by the header")
            continue
        ret, params = declared[name]
        if len(params) != len(argtypes):
            wrong.append(f"{name}: {len(argtypes)} argument types for {len(params)} parameters")
            continue
        wrong += [f"{name}: parameter {pname} is {ptype!r}, bound as {a.__name__}"
                  for (ptype, pname), a in zip(params, argtypes) if _class_of_c(ptype) != _class_of(a)]
        restype = capi._RESTYPES.get(name, ctypes.c_int)
        if {"int": ctypes.c_int, "void": None, "const char *": ctypes.c_char_p, "almpc_handle *": ctypes.c_void_p}[ret] is not restype:
            wrong.append(f"{name}: returns {ret!r}, bound as {restype}")
    assert not wrong, "\n".join(wrong)
    assert set(NOT_BOUND) <= set(declared) and not set(NOT_BOUND) & set(table)
    assert sorted(set(declared) - set(table)) == sorted(NOT_BOUND)
