"""CPU: the many-link call table's item packing against include/grdma_amd.h and the compiler, and its prototype in the one
ABI table."""
import os
import re
import subprocess

import pytest

from tests.emu_harness import CLANG, ROOT
from tests.h2_links_calls_lib import ITEM_FIELDS, item_dtype

HEADER = os.path.join(ROOT, "include", "grdma_amd.h")


def header_members(struct):
    """the member names of a struct of the header, in order (tests/test_abi_table.py's reading of a body)"""
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    body = re.search(r"struct\s+%s\s*\{([^{}]*)\}" % struct, src).group(1)
    return [re.findall(r"\w+", d)[-1] for decl in body.split(";") if decl.strip() for d in decl.split(",")]


def test_item_columns_equal_the_header_s_members():
    from grpc_rdma_amd import h2dev
    assert list(ITEM_FIELDS) == header_members("grdma_h2_calls_item") == list(h2dev.CALLS_ITEM) and len(ITEM_FIELDS) == 14
    dt = item_dtype()
    assert dt.itemsize == 112 and list(dt.names) == list(ITEM_FIELDS) and all(dt.fields[n] == (dt.fields[n][0], 8 * k) for k, n in enumerate(dt.names))


@pytest.mark.skipif(not os.path.exists(CLANG), reason="needs the ROCm clang++ as host compiler")
def test_item_layout_equals_the_compiler_s(tmp_path):
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "grdma_amd.h"', "int main() {",
             '  printf("size %zu\\n", sizeof(grdma_h2_calls_item));']
    for name in ITEM_FIELDS:
        lines.append('  printf("%s %%zu %%zu\\n", offsetof(grdma_h2_calls_item, %s), sizeof(((grdma_h2_calls_item*)0)->%s));' % (name, name, name))
    lines += ["  return 0;", "}"]
    src, exe = tmp_path / "item.cc", tmp_path / "item"
    src.write_text("\n".join(lines) + "\n")
    subprocess.run([CLANG, "-std=c++17", "-Wno-invalid-offsetof", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True, capture_output=True, text=True)
    got = {}
    for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines():
        key, *numbers = line.split()
        got[key] = tuple(int(x) for x in numbers)
    dt = item_dtype()
    want = {"size": (dt.itemsize,)}
    for name in dt.names:
        want[name] = (dt.fields[name][1], dt.fields[name][0].itemsize)
    assert got == want and got["size"] == (112,)


def test_the_abi_table_carries_the_prototype():
    import ctypes as C
    from grpc_rdma_amd import _abi
    restype, argtypes = _abi.SIGNATURES["grdma_h2_calls_step_batch"]
    assert restype is C.c_int and list(argtypes) == [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint64)]
    assert "grdma_h2_calls_step_batch" not in _abi.UNDECLARED
