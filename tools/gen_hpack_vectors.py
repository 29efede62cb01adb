#!/usr/bin/env python3
"""Writes tests/golden/h2_hpack_vectors.json: a subset of the cases of tests/test_h2_hpack_model.py with nghttp2's
answers, so that the model of tests/h2_hpack_model.py is pinned where libnghttp2 cannot be loaded -- header lists through
its deflater with what its inflater made of every block, the size of its dynamic table behind every block and the table
itself behind the last; the captured blocks; the malformed blocks it rejects.  `--data` rewrites
tests/h2_hpack_data.py (the model's tables) from the library instead.  Needs libnghttp2."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import h2_hpack_lib as L  # noqa: E402

VECTORS = os.path.join(ROOT, "tests", "golden", "h2_hpack_vectors.json")
DATA = os.path.join(ROOT, "tests", "h2_hpack_data.py")
SEEDS = range(2)


def static_from_nghttp2():
    inf, out = L.Inflater(), [(b"", b"")]
    for i in range(1, 62):
        (n, v, _), = inf.inflate(bytes([0x80 | i]))
        out.append((n, v))
    return out


def inflated(blocks):
    """the blocks through one inflater -> per block {hex, fields, entries, size}, the last one with the table; fields None
    where it rejects the block"""
    inf, out = L.Inflater(), []
    for b in blocks:
        got = inf.inflate(b)
        table, size = inf.table()
        out.append({"hex": b.hex(), "fields": None if got is None else [[n.hex(), v.hex(), int(x)] for n, v, x in got],
                    "entries": len(table), "size": size})
        if got is None:
            break
    out[-1]["table"] = [[n.hex(), v.hex()] for n, v in table]
    return out


def vectors():
    return {
        "source": "tools/gen_hpack_vectors.py over libnghttp2's nghttp2_hd_deflate_* / nghttp2_hd_inflate_*",
        "deflated": [inflated([b for b, _, _ in L.deflated_sequence(s, 3)]) for s in SEEDS],
        "capture": inflated([b for _, b in L.capture_blocks()]),
        "malformed": [{"what": what, "blocks": inflated(front + [bad])} for what, front, bad in L.malformed()],
    }


def dump(v, depth=0):
    """JSON with a line per block: lists of lists and dicts of lists are broken, a block (a dict with "hex") is not"""
    if isinstance(v, dict) and "hex" not in v:
        return "{\n" + ",\n".join("%s: %s" % (json.dumps(k), dump(x, depth + 1)) for k, x in v.items()) + "\n}"
    if isinstance(v, list) and v and isinstance(v[0], (list, dict)) and depth < 3:
        return "[\n" + ",\n".join(dump(x, depth + 1) for x in v) + "\n]"
    return json.dumps(v, separators=(",", ":"))


def write_data():
    codes, static = L.huffman_from_nghttp2(), static_from_nghttp2()
    out = ['"""The data of the HPACK model (tests/h2_hpack_model.py): the Huffman code of RFC 7541 Appendix B as (code, bits) per\n'
           'symbol, 256 = EOS, and the static table of Appendix A as (name, value), index 0 unused.  Written by\n'
           'tools/gen_hpack_vectors.py --data from nghttp2\'s tables; tests/test_h2_hpack_model.py pins both against the library."""',
           "HUFFMAN = ["]
    for k in range(0, 257, 8):
        out.append("    " + ", ".join("(0x%x, %d)" % c for c in codes[k:k + 8]) + ",")
    out += ["]", "STATIC = ["] + ["    (%r, %r)," % e for e in static] + ["]"]
    with open(DATA, "w") as f:
        f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    if L.NGHTTP2 is None:
        sys.exit(L.NO_NGHTTP2)
    if "--data" in sys.argv:
        write_data()
        print("wrote", DATA)
    else:
        with open(VECTORS, "w") as f:
            f.write(dump(vectors()) + "\n")
        print("wrote", VECTORS, os.path.getsize(VECTORS), "bytes")
