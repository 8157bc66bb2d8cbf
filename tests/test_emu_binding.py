"""tests/emu.py's PROTOTYPES against the emulator it declares: every
`extern "C"` definition of csrc/ikg_host_emu.hip (read as text, as
tests/test_capi.py reads include/ikgrasp.h) has a row with the same number of
arguments and the same type class per argument and for the return value, and
every row resolves in the built library."""
import ctypes as C
import os
import re

import pytest

import emu as host_emu
from conftest import PKG

SOURCE = os.path.join(PKG, "csrc", "ikg_host_emu.hip")
DEFINITION = re.compile(r'extern "C" ([\w ]+?)\s*\*?\s*(ikg_emu_\w+)\(([^)]*)\)\s*\{')


# `long long` and int64_t are one class: ctypes' c_longlong is its c_int64
SCALARS = {"int64_t": "i64", "long long": "i64", "int": "i32", "int32_t": "i32", "double": "f64", "void": "void"}


def type_class(decl, named=False):
    """"ptr", "i64", "i32", "f64" or "void" of a C return type, or of a parameter's
    declaration (named: its last word is the parameter's name; `int32_t out[8]` is a pointer)"""
    if "*" in decl or "[" in decl:
        return "ptr"
    words = [w for w in decl.split() if w != "const"]
    return SCALARS[" ".join(words[:-1] if named else words)]


def ctype_class(ct):
    if ct is None:
        return "void"
    if issubclass(ct, C._Pointer):
        return "ptr"
    return {C.c_void_p: "ptr", C.c_int: "i32", C.c_int32: "i32", C.c_int64: "i64", C.c_longlong: "i64", C.c_double: "f64"}[ct]


def definitions():
    """name -> (return type, [parameter declarations]) of the source"""
    with open(SOURCE) as f:
        text = f.read()
    out = {}
    for ret, name, params in DEFINITION.findall(text):
        assert name not in out, name
        out[name] = (ret.strip(), [" ".join(p.split()) for p in params.split(",")])
    return out


def same_class(decl, ct, named=False):
    """A C return type or parameter declaration against a ctype."""
    return type_class(decl, named) == ctype_class(ct)


def test_the_source_has_the_29_exports_the_table_lists():
    defs = definitions()
    assert len(defs) == 29
    assert set(defs) == set(host_emu.PROTOTYPES)


@pytest.mark.parametrize("name", sorted(host_emu.PROTOTYPES))
def test_row_matches_the_definition(name):
    ret, params = definitions()[name]
    restype, argtypes = host_emu.PROTOTYPES[name]
    assert len(argtypes) == len(params), (name, params)
    assert same_class(ret, restype), (name, "return", ret, restype)
    for k, (decl, ct) in enumerate(zip(params, argtypes)):
        assert same_class(decl, ct, named=True), (name, k, decl, ct)


def test_type_classes():
    """The classifier itself: what it calls each C spelling in the source, and that it tells the
    ctypes apart that a wrong row would confuse."""
    assert [type_class(t) for t in ("const double*", "int32_t", "int", "int64_t", "double", "long long", "void",
                                    "const ikg_model_desc*")] == \
        ["ptr", "i32", "i32", "i64", "f64", "i64", "void", "ptr"]
    assert [type_class(t, named=True) for t in ("int32_t out[8]", "const void* q", "int64_t B", "int on")] == \
        ["ptr", "ptr", "i64", "i32"]
    assert ctype_class(C.c_int) == "i32" and ctype_class(C.c_int64) == "i64" and ctype_class(C.c_void_p) == "ptr"
    assert ctype_class(C.POINTER(C.c_double)) == "ptr" and ctype_class(None) == "void"
    assert not same_class("int64_t", C.c_int) and not same_class("int", C.c_int64) and not same_class("double", C.c_int64)
    assert not same_class("const double*", C.c_int64) and not same_class("void", C.c_int) and not same_class("int", None)
    assert same_class("long long", C.c_longlong) and same_class("int64_t", C.c_int64) and C.sizeof(C.c_longlong) == 8


def test_every_row_resolves_in_the_built_library():
    lib = host_emu.load_or_skip()
    for name, (restype, argtypes) in host_emu.PROTOTYPES.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name
