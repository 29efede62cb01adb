"""CPU: the ctypes side of the C ABI (grpc-rdma_amd/_abi.py) held to include/grdma_amd.h.

Functions: SIGNATURES names exactly the functions the header declares, and the return and every parameter of each entry
is of the header's class (pointer / i32 / u32 / i64 / u64 / f64 / void), in number and order.  Structures: every class in
STRUCTS has the size, the field names and the field offsets and sizes of the header struct it mirrors, as the host
compiler lays that struct out.  A C type or a ctypes type this file does not know is a failure, not a default."""
import ctypes as C
import os
import re
import subprocess

import pytest

from grpc_rdma_amd import _abi, _lib, h2dev, stream
from tests.emu_harness import CLANG, ROOT

HEADER = os.path.join(ROOT, "include", "grdma_amd.h")
C_CLASS = {"int": "i32", "int32_t": "i32", "uint32_t": "u32", "int64_t": "i64", "uint64_t": "u64", "double": "f64"}
CTYPES_CLASS = {C.c_int32: "i32", C.c_uint32: "u32", C.c_int64: "i64", C.c_uint64: "u64", C.c_double: "f64",
                C.c_void_p: "pointer", C.c_char_p: "pointer"}


def header_text():
    """the header without comments and preprocessor lines"""
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    src = re.sub(r"//[^\n]*", "", src)
    return "\n".join(line for line in src.splitlines() if not line.lstrip().startswith("#"))


def c_class(decl, is_return=False):
    """the class of a C return type, or of a parameter declaration with its name"""
    if "*" in decl or "[" in decl:
        return "pointer"
    words = [w for w in decl.split() if w != "const"]
    if not is_return and len(words) > 1:
        words.pop()  # (the parameter's name)
    if is_return and words == ["void"]:
        return "void"
    assert len(words) == 1 and words[0] in C_CLASS, "a C type this test does not know: %r" % decl
    return C_CLASS[words[0]]


def ctypes_class(t, is_return=False):
    if t is None and is_return:
        return "void"
    if isinstance(t, type) and issubclass(t, (C._Pointer, C.Array)):
        return "pointer"
    assert t in CTYPES_CLASS, "a ctypes type this test does not know: %r" % (t,)
    return CTYPES_CLASS[t]


def declarations():
    """{name: (class of the return, [class of each parameter])} of every `ret name(args);` in the header"""
    out = {}
    for ret, name, args in re.findall(r"([A-Za-z_][\w\s\*]*?[\s\*])(grdma_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", header_text()):
        args = args.strip()
        params = [] if args in ("", "void") else [c_class(a.strip()) for a in args.split(",")]
        assert name not in out, "%s is declared twice" % name
        out[name] = (c_class(ret.strip(), is_return=True), params)
    return out


def signature_errors(table, decls):
    """what in the prototype table disagrees with the declarations, one line each"""
    errors = ["%s: in the table, not in the header" % n for n in sorted(set(table) - set(decls))]
    errors += ["%s: in the header, not in the table" % n for n in sorted(set(decls) - set(table))]
    for name in sorted(set(table) & set(decls)):
        res, args = table[name]
        got = (ctypes_class(res, is_return=True), [ctypes_class(a) for a in args])
        if got != decls[name]:
            errors.append("%s: the table says %r, the header %r" % (name, got, decls[name]))
    return errors


def test_the_parser_reads_every_declaration():
    names = set(re.findall(r"\b(grdma_[a-z0-9_]+)\s*\(", header_text()))
    assert len(names) >= 200
    assert set(declarations()) == names


def test_prototype_table_equals_the_header(built):
    assert signature_errors(_abi.SIGNATURES, declarations()) == []
    assert not set(_abi.UNDECLARED) & set(_abi.SIGNATURES)
    assert _lib.load().grdma_abi_version() == 2


def test_a_wrong_entry_is_found():
    """the comparison itself: a return of the wrong width, a parameter of the wrong class, one too few, a stray name"""
    decls = declarations()
    for name, wrong in (("grdma_h2_last_kernel_us", (C.c_int64, [])),
                        ("grdma_pair_watch_hits", (C.c_int, [C.c_void_p])),
                        ("grdma_pair_arm_read", (C.c_int, [C.c_void_p, C.c_uint32])),
                        ("grdma_pair_arm_read", (C.c_int, [C.c_void_p])),
                        ("grdma_pair_destroy", (C.c_int, [C.c_void_p]))):
        errors = signature_errors(dict(_abi.SIGNATURES, **{name: wrong}), decls)
        assert len(errors) == 1 and errors[0].startswith(name + ":"), (name, errors)
    assert len(signature_errors(dict(_abi.SIGNATURES, **_abi.UNDECLARED), decls)) == len(_abi.UNDECLARED)
    with pytest.raises(AssertionError, match="does not know"):
        signature_errors(dict(_abi.SIGNATURES, grdma_init=(C.c_int, [C.c_int16])), decls)


def test_the_old_modules_still_export_their_names():
    for mod, names in ((_lib, ("Slice", "ReadSlice", "PairState", "Config", "SIGNATURES")), (stream, ("StreamResult",)),
                       (h2dev, [c.__name__ for c in _abi.STRUCTS if c.__name__.startswith("H2")])):
        for n in names:
            assert getattr(mod, n) is getattr(_abi, n)
    assert len(_abi.STRUCTS) == 20 and len(set(_abi.STRUCTS.values())) == 20


def header_fields():
    """{struct name: [field names in order]} of every struct the header defines"""
    out = {}
    for name, body in re.findall(r"struct\s+(grdma_\w+)\s*\{([^{}]*)\}", header_text()):
        out[name] = [re.findall(r"\w+", re.sub(r"\[[^\]]*\]", "", d))[-1]
                     for decl in body.split(";") if decl.strip() for d in decl.split(",")]
    return out


def test_structure_field_names_equal_the_header():
    fields = header_fields()
    for cls, name in _abi.STRUCTS.items():
        assert [n for n, _ in cls._fields_] == fields[name], name


@pytest.mark.skipif(not os.path.exists(CLANG), reason="needs the ROCm clang++ as host compiler")
def test_structure_layouts_equal_the_compiler_s(tmp_path):
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "grdma_amd.h"', "int main() {"]
    for cls, name in _abi.STRUCTS.items():
        lines.append('  printf("%s %%zu\\n", sizeof(%s));' % (name, name))
        for field, _ in cls._fields_:
            lines.append('  printf("%s.%s %%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s*)0)->%s));'
                         % (name, field, name, field, name, field))
    lines += ["  return 0;", "}"]
    src, exe = tmp_path / "layout.cc", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    subprocess.run([CLANG, "-std=c++17", "-Wno-invalid-offsetof", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True, capture_output=True, text=True)
    got = {}
    for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines():
        key, *numbers = line.split()
        got[key] = tuple(int(x) for x in numbers)
    want = {}
    for cls, name in _abi.STRUCTS.items():
        want[name] = (C.sizeof(cls),)
        for field, _ in cls._fields_:
            want["%s.%s" % (name, field)] = (getattr(cls, field).offset, getattr(cls, field).size)
    assert got == want
