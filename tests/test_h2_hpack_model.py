"""The HPACK model (tests/h2_hpack_model.py) against an independent implementation before a device test trusts it:
nghttp2's public hd API through ctypes (tests/h2_hpack_lib.py), and -- so that the model is pinned where the library
cannot be loaded -- nghttp2's answers as tools/gen_hpack_vectors.py wrote them into tests/golden/h2_hpack_vectors.json."""
import json
import os
from fractions import Fraction

import pytest

from tests import h2_hpack_lib as L
from tests.h2_hpack_model import HUFFMAN, STATIC, HpackError, HpackTable

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
needs_nghttp2 = pytest.mark.skipif(L.NGHTTP2 is None, reason=L.NO_NGHTTP2)
VECTORS = json.load(open(os.path.join(ROOT, "tests", "golden", "h2_hpack_vectors.json")))


def decode(table, block):
    """-> [(name, value, never indexed)], or None where the model rejects the block"""
    try:
        return [(n, v, rep == 3) for n, v, rep in table.decode_block(block)]
    except HpackError:
        return None


def test_the_huffman_code_is_complete():
    assert len(HUFFMAN) == 257 and HUFFMAN[256] == (0x3fffffff, 30)
    assert (min(n for _, n in HUFFMAN), max(n for _, n in HUFFMAN)) == (5, 30)
    assert sum(Fraction(1, 1 << n) for _, n in HUFFMAN) == 1  # Kraft: every bit string is a code word's prefix
    assert len(STATIC) == 62 and STATIC[2] == (b":method", b"GET") and STATIC[61] == (b"www-authenticate", b"")


@needs_nghttp2
def test_the_tables_equal_nghttp2s():
    assert HUFFMAN == L.huffman_from_nghttp2()
    inf = L.Inflater()
    for i in range(1, 62):
        assert inf.inflate(bytes([0x80 | i])) == [STATIC[i] + (False,)]


def test_the_committed_tables_header_is_what_the_generator_writes():
    import importlib.util
    spec = importlib.util.spec_from_file_location("gen_hpack_tables", os.path.join(ROOT, "tools", "gen_hpack_tables.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    assert open(gen.PATH).read() == gen.text()
    words = gen.automaton()
    assert len(words) == 4096 and all((w & 0xff) < 256 for w in words)
    # the automaton decodes what the encoder of the library wrote, and stops where the model stops
    every = bytes(range(256))
    state, out = 0, bytearray()
    for b in L.huff(every):
        for nibble in (b >> 4, b & 15):
            w = words[16 * state + nibble]
            assert not w & gen.FAIL
            if w & gen.EMIT:
                out.append(w >> 16)
            state = w & 0xff
    assert bytes(out) == every and w & gen.ACCEPT


@needs_nghttp2
def test_two_thousand_header_lists_through_nghttp2s_deflater():
    n = 0
    for seed in range(500):
        table, inf = HpackTable(), L.Inflater()
        for block, headers, never in L.deflated_sequence(seed):
            want = [(name, value, i in never) for i, (name, value) in enumerate(headers)]
            assert decode(table, block) == inf.inflate(block) == want, (seed, block.hex())
            assert (table.entries, table.size) == inf.table(), (seed, block.hex())
            n += 1
    assert n == 2000


@needs_nghttp2
def test_blocks_of_the_librarys_own_encoder():
    for seed in range(300):
        table, inf = HpackTable(), L.Inflater()
        for block, headers in L.own_sequence(seed):
            got = decode(table, block)
            assert got is not None and [f[:2] for f in got] == headers, (seed, block.hex())
            assert got == inf.inflate(block), (seed, block.hex())
            assert (table.entries, table.size) == inf.table(), (seed, block.hex())


@needs_nghttp2
def test_the_captured_blocks():
    table, inf = HpackTable(), L.Inflater()
    blocks = L.capture_blocks()
    assert [len(b) for _, b in blocks] == [234, 9, 9, 9, 68] and blocks[1][1] == bytes.fromhex("c4c38386c2c1c0bfbe")
    for _, block in blocks:
        got = decode(table, block)
        assert got == inf.inflate(block) and len(got) == 9
        assert (table.entries, table.size) == inf.table()


@needs_nghttp2
@pytest.mark.parametrize("case", L.malformed(), ids=lambda c: c[0])
def test_malformed_blocks_are_rejected_by_both(case):
    what, front, bad = case
    table, inf = HpackTable(), L.Inflater()
    for block in front:
        assert decode(table, block) == inf.inflate(block) != None  # noqa: E711
    assert decode(table, bad) is None and inf.inflate(bad) is None


def _replay(blocks):
    table = HpackTable()
    for b in blocks:
        got = decode(table, bytes.fromhex(b["hex"]))
        assert (None if got is None else [[n.hex(), v.hex(), int(x)] for n, v, x in got]) == b["fields"], b["hex"]
        if got is not None:
            assert (len(table.entries), table.size) == (b["entries"], b["size"]), b["hex"]
        if "table" in b:
            assert [[n.hex(), v.hex()] for n, v in table.entries] == b["table"], b["hex"]


def test_the_golden_vectors():
    assert len(VECTORS["deflated"]) == 2 and len(VECTORS["capture"]) == 5
    for seq in VECTORS["deflated"] + [VECTORS["capture"]]:
        assert all(b["fields"] is not None for b in seq)
        _replay(seq)
    assert len(VECTORS["malformed"]) == 9
    for case in VECTORS["malformed"]:
        assert case["blocks"][-1]["fields"] is None and all(b["fields"] is not None for b in case["blocks"][:-1]), case["what"]
        _replay(case["blocks"])


# ---- the sweep of tests/test_zz_gpu_h2_hpack_sweep.py: its witnesses, and its block sequences through nghttp2 --------------
PER_FAMILY = {"01": 20, "02": 22, "03": 16, "04": 10, "05": 6, "06": 60, "07": 39, "08": 61, "09": 10, "10": 6}


def test_every_case_of_the_hpack_sweep_shows_its_witness():
    import collections
    from tests import h2_hpack_sweep_lib as S
    cs = S.check_cases()
    assert collections.Counter(c["fam"] for c in cs) == PER_FAMILY and len(cs) == sum(PER_FAMILY.values()) == 250
    assert set(PER_FAMILY) == set(S.FAMILIES) and all(c["edge"] and c["key"] for c in cs)
    subset = S.emu_subset()
    assert {S.by_id(cid)["fam"] for cid in subset} == set(S.FAMILIES) and all(cid in subset for cid in S.CAUGHT_ALONE)
    # what the subset always holds: the chunk path, the ring's wrap at 2048, a byte-ring straddle, 2^32 - 1, an index >= 2^24
    sims = {cid: S.simulate(S.by_id(cid)) for cid in subset}
    assert any(st[1] == 0 for sim in sims.values() for s in sim for st in s.get("steps", ()))
    assert any(s.get("ins0", 0) < S.RING < s.get("ins1", 0) for sim in sims.values() for s in sim)
    assert any(s.get("straddles") for sim in sims.values() for s in sim)
    assert any(cid.endswith("_2p32m1") for cid in subset) and any(S.by_id(cid)["key"].startswith("big_") for cid in subset)
    assert not any(cid[:2] in ("04", "05", "07") for cid in S.NGHTTP2_DIFFERS) and set(S.NGHTTP2_DIFFERS) <= set(S._BY_ID)


@needs_nghttp2
@pytest.mark.parametrize("fam", ["01", "02", "04", "05", "06", "07", "09"])
def test_the_sweeps_block_sequences_through_nghttp2(fam):
    """accept or reject, the fields with their never-indexed flag and the dynamic table; error codes are not compared"""
    import copy
    from tests import h2_hpack_sweep_lib as S
    assert fam in S.PINNED
    n = 0
    for c in (c for c in S.CASES if c["fam"] == fam):
        table, inf = HpackTable(c["setting"]), L.Inflater(c["setting"])
        for kind, x in S.pin_sequence(c):
            if kind == "resize":
                table.set_setting(x)
                inf.change_table_size(x)
                assert (table.entries, table.size) == inf.table(), c["id"]
                continue
            good = copy.deepcopy(table)
            got, theirs = decode(table, x), inf.inflate(x)
            if theirs is None and got is not None and c["id"] in S.NGHTTP2_DIFFERS:
                break
            assert (got is None) == (theirs is None), (c["id"], x[:64].hex())
            if got is None:
                table = good
                break  # (the decoder is dead behind a failed block)
            assert got == theirs, (c["id"], x[:64].hex())
            assert (table.entries, table.size) == inf.table(), (c["id"], x[:64].hex())
            n += 1
    assert n > 0
