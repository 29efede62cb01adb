"""CPU: the many-link metadata reader's item packing against include/grdma_amd.h, and the batch model of
tests/h2_links_meta_lib.py -- ONE MetaModel read per item in item order, ONE call -- over the cases of the device tests
that move the counters item by item (nine links over three calls, trouble that stays with its item)."""
import os
import re
import subprocess

import pytest

from tests.emu_harness import CLANG, ROOT
from tests.h2_hpenc_model import pack
from tests.h2_links_meta_lib import ITEM_FIELDS, item_dtype, model_batch
from tests.h2_meta_lib import PATH, request, trailers
from tests.h2_meta_model import BAD_INPUT, ERR_STREAM, STAT_KEYS, MetaModel

HEADER = os.path.join(ROOT, "include", "grdma_amd.h")
BIG = 1 << 40
NOWHERE = b"/svc/none"


def header_members(struct):
    """the member names of a struct of the header, in order (tests/test_abi_table.py's reading of a body)"""
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    body = re.search(r"struct\s+%s\s*\{([^{}]*)\}" % struct, src).group(1)
    return [re.findall(r"\w+", d)[-1] for decl in body.split(";") if decl.strip() for d in decl.split(",")]


def test_item_columns_equal_the_header_s_members():
    from grpc_rdma_amd import h2dev
    assert list(ITEM_FIELDS) == header_members("grdma_h2_meta_item") == list(h2dev.META_ITEM)
    dt = item_dtype()
    assert dt.itemsize == 80 and list(dt.names) == list(ITEM_FIELDS) and all(dt.fields[n] == (dt.fields[n][0], 8 * k) for k, n in enumerate(dt.names))


@pytest.mark.skipif(not os.path.exists(CLANG), reason="needs the ROCm clang++ as host compiler")
def test_item_layout_equals_the_compiler_s(tmp_path):
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "grdma_amd.h"', "int main() {",
             '  printf("size %zu\\n", sizeof(grdma_h2_meta_item));']
    for name in ITEM_FIELDS:
        lines.append('  printf("%s %%zu %%zu\\n", offsetof(grdma_h2_meta_item, %s), sizeof(((grdma_h2_meta_item*)0)->%s));' % (name, name, name))
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
    assert got == want and got["size"] == (80,)


def mixed(n, refused=(), malformed=(), first=1):
    return [(first + 2 * k, k & 1, request(NOWHERE) if k in refused else request(drop=(b":path",)) if k in malformed else request())
            for k in range(n)]


def stats(m):
    return tuple(m.stats[k] for k in STAT_KEYS)


def test_nine_links_over_three_calls_count_as_three_calls():
    m, one = MetaModel((PATH,)), MetaModel((PATH,))
    total = [0] * 6
    for n in range(3):
        tables = [pack(mixed(3 * i + n, refused=range(i % 4, 3 * i + n, 4), malformed=range(i % 5 + 1, 3 * i + n, 5)) + [(999, 1, trailers())])
                  for i in range(9)]
        exp = model_batch(m, tables, [(BIG, BIG)] * 9)
        assert all(e[3] is None for e in exp)
        total = [t + sum(e[2][k] for e in exp) for k, t in enumerate(total)]
        assert stats(m) == (n + 1,) + tuple(total)
        # ... which is what nine single reads count, apart from the calls
        for t in tables:
            one.read(*t, BIG, BIG)
        assert stats(one)[0] == 9 * (n + 1) and stats(one)[1:] == stats(m)[1:]


def test_items_that_are_not_read_count_nowhere():
    m = MetaModel((PATH,))
    blocks, fields, arena = pack(mixed(12))
    bad = ([(0,) + blocks[0][1:]] + blocks[1:], fields, arena)
    l3, g5, g6 = pack(mixed(21, refused=range(0, 21, 2))), pack(mixed(17, refused=(3, 16), malformed=(9,)) + [(77, 1, trailers())]), pack(mixed(2))
    exp = model_batch(m, [g5, l3, bad, g6, l3], [(BIG, BIG), (20, BIG), (BIG, BIG), (BIG, BIG), (BIG, 10)])
    assert [e[3] for e in exp] == [None, "capacity", "invalid", None, "capacity"]
    assert exp[2][2] == (0, 0, 0, 0, 0, 0, BAD_INPUT | ERR_STREAM << 8, 0) and exp[1][2] == exp[4][2] == (21, 21, 0, 0, 11, 0, 0, 1)
    assert stats(m) == (1, 20, 19, 0, 1, 2, 1)  # the two good items, ONE call
    before = stats(m)
    exp = model_batch(m, [bad, l3], [(BIG, BIG), (21, 10)])  # a batch in which no item is read
    assert [e[3] for e in exp] == ["invalid", "capacity"] and stats(m) == before
    exp = model_batch(m, [l3], [(21, 11)])  # exactly the need: one item, one call
    assert exp[0][3] is None and stats(m) == (2, 41, 40, 0, 1, 13, 1)
