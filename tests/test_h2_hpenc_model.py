"""The model of the header-block encoder (tests/h2_hpenc_model.py) against three references that do not share its code:
the header blocks RFC 7541 prints in Appendix C.4 and C.6 (tests/golden/h2_hpenc_vectors.json), the decoder's model
(tests/h2_hpack_model.py: every block decodes back to its list, table for table), and nghttp2's inflater."""
import json
import os
import random

import pytest

from tests import h2_hpack_lib as L
from tests import h2_hpenc_model as M
from tests.h2_hpack_model import STATIC, HpackTable, split

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VECTORS = json.load(open(os.path.join(ROOT, "tests", "golden", "h2_hpenc_vectors.json")))
needs_nghttp2 = pytest.mark.skipif(L.NGHTTP2 is None, reason=L.NO_NGHTTP2)


def _gen():
    import importlib.util
    spec = importlib.util.spec_from_file_location("gen_hpack_tables", os.path.join(ROOT, "tools", "gen_hpack_tables.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    return gen


def test_both_committed_tables_headers_are_what_the_generator_writes():
    gen = _gen()
    assert open(gen.PATH).read() == gen.text()
    assert open(gen.ENC_PATH).read() == gen.enc_text()


@pytest.mark.parametrize("which", ["C.4", "C.6"])
def test_the_rfcs_header_blocks_byte_for_byte(which):
    v = VECTORS[which]
    m, dec = M.HpencModel(v["table_size"]), HpackTable(v["table_size"])
    for k, b in enumerate(v["blocks"]):
        hs = [(n.encode(), x.encode(), 1) for n, x in b["headers"]]
        # (the printed block decodes to the printed list: the vector itself is held against the decoder's model)
        assert [(n, x) for n, x, _ in dec.decode_block(bytes.fromhex(b["hex"]))] == [(n, x) for n, x, _ in hs]
        wire, bw, res, err = m.encode(*M.pack([(2 * k + 1, 0, hs)]), 1 << 20, 8)
        assert err is None and M.deframe(wire) == [(2 * k + 1, 0, bytes.fromhex(b["hex"]))], (wire[9:].hex(), b["hex"])
        assert bw == [(0, len(wire), 1)] and res[:3] == (1, 1, len(wire))
        assert m.table.entries == [(n.encode(), x.encode()) for n, x in b["table"]] == dec.entries
        assert m.table.size == b["table_bytes"] == dec.size


def expected_rep(table, name, value, hint):
    """the representation a hint asks for, from the table in front of the field"""
    live = (name, value) in STATIC[1:] or (name, value) in table.entries
    if hint == 3:
        return 3
    return 0 if live else (1 if hint < 2 else 2)


def sequences():
    """2000 header lists in 500 sequences at table sizes 0, 100 and 4096 with changes in between ->
    [(seed, [(size to set in front or None, headers with hints)])]"""
    out = []
    for seed in range(500):
        rng = random.Random(seed)
        seq = []
        for k in range(4):
            size = rng.choice([0, 100, 4096]) if (k == 0 or rng.random() < 0.3) else None  # (in front of block k)
            seq.append((size, [(n, v, rng.choice([0, 1, 1, 1, 2, 3])) for n, v in L.random_headers(rng)]))
        out.append((seed, seq))
    return out


def run_sequences(make_decoder, decode, check_table):
    """every block of the sequences through the model and a decoder of 4096 bytes at the start (what both sides hold
    before any SETTINGS; the sizes are set through set_peer, the first one too) -> per block (seed, k, headers, block,
    decoded, the model, the table in front of the block)"""
    n = 0
    for seed, seq in sequences():
        m, dec = M.HpencModel(4096), make_decoder()
        for k, (size, hs) in enumerate(seq):
            if size is not None:
                if seed % 3 == 0:  # (lowered then raised, or set and set back)
                    m.set_peer(random.Random(seed * 7 + k).choice([0, 100, 4096]), 16384)
                m.set_peer(size, 16384)
            before = HpackTable(4096)
            before.max_size, before.entries, before.size = m.table.max_size, list(m.table.entries), m.table.size
            wire, bw, res, err = m.encode(*M.pack([(1, 0, hs)]), 1 << 20, 8)
            assert err is None
            (stream, es, block), = M.deframe(wire)
            got = decode(dec, block)
            assert got is not None, (seed, k)
            assert [(a, b) for a, b, _ in got] == [(a, b) for a, b, _ in hs], (seed, k)
            check_table(dec, m.table)
            yield seed, k, hs, block, got, m, before
            n += 1
    assert n == 2000


def test_two_thousand_lists_round_trip_through_the_decoders_model():
    def check(dec, t):
        assert (dec.entries, dec.size, dec.max_size) == (t.entries, t.size, t.max_size)

    seen = set()
    names = [e[0] for e in STATIC[1:]]
    for seed, k, hs, block, got, m, t in run_sequences(lambda: HpackTable(4096), lambda d, b: d.decode_block(b), check):
        # the representation each hint asks for, and the index the matching rules ask for: the block's fields replayed
        # against the table in front of each
        reps = []
        for f in split(block, 4096):
            if f[0] == "size":
                assert not reps
                t.apply([f])
                continue
            name, value, hint = hs[len(reps)]
            want = expected_rep(t, name, value, hint)
            assert f[0] == want == m.last_reps[len(reps)], (seed, k, len(reps), f, want)
            if f[0] == 0:
                assert f[1] == (STATIC.index((name, value)) if (name, value) in STATIC[1:] else 62 + t.entries.index((name, value)))
            elif f[1]:
                assert f[1] == (1 + names.index(name) if name in names else 62 + [e[0] for e in t.entries].index(name))
            else:
                assert name not in names + [e[0] for e in t.entries]
            t.apply([f])
            reps.append(f[0])
            seen.add((hint, f[0]))
        assert len(reps) == len(hs)
    assert seen >= {(0, 0), (0, 1), (1, 0), (1, 1), (2, 0), (2, 2), (3, 3)}


@needs_nghttp2
def test_the_same_blocks_through_nghttp2s_inflater():
    def check(inf, t):
        assert inf.table() == (t.entries, t.size)

    for seed, k, hs, block, got, m, _ in run_sequences(L.Inflater, lambda d, b: d.inflate(b), check):
        assert [nv for _, _, nv in got] == [hint == 3 for _, _, hint in hs], (seed, k)


def test_strings_go_huffman_where_that_is_not_longer():
    for data in (b"", b"a", b"!", b"307", b"www.example.com", bytes(range(256)), b"\x00" * 9, b"0" * 8, b"0" * 7, b"aaaaaaaa"):
        s = M.enc_str(data)
        coded = bool(s[0] & 0x80)
        assert coded == (len(data) > 0 and M.huffman_len(data) <= len(data))
        assert L.enc_str(data, h=coded) == s
    assert M.enc_str(b"0")[0] & 0x80 and M.enc_str(b"307") == bytes.fromhex("83640eff") and M.enc_str(b"") == b"\x00"
    assert M.huffman_len(b"\x00") == 2 and not M.enc_str(b"\x00")[0] & 0x80


def test_the_hash_is_fnv1a_and_the_colliding_pairs_collide():
    from tests.h2_hpenc_lib import FULL_COLLISION, NAME_COLLISION
    assert M.hash_bytes(b"") == 0x811c9dc5 and M.hash_bytes(b"a") == 0xe40c292c and M.hash_bytes(b"foobar") == 0xbf9cf968
    (n1, v1), (n2, v2) = FULL_COLLISION
    assert (n1, v1) != (n2, v2) and M.full_hash(n1, v1) == M.full_hash(n2, v2) and len(n1) == len(n2) and len(v1) == len(v2)
    a, b = NAME_COLLISION
    assert a != b and len(a) == len(b) and M.name_hash(a) == M.name_hash(b)


def test_size_updates_of_the_model():
    m = M.HpencModel(4096)
    assert m.updates() == []
    m.set_peer(100, 16384)
    assert m.updates() == [100]
    m.set_peer(200, 16384)
    assert m.updates() == [100, 200]
    m.set_peer(0, 16384)
    m.set_peer(4096, 16384)
    assert m.updates() == [0, 4096]
    wire, _, res, _ = m.encode(*M.pack([(1, 0, [(b"a", b"b")])]), 1 << 20, 8)
    assert wire[9:12] == b"\x20\x3f\xe1" and m.updates() == []
    m.set_peer(8192, 16384)
    m.set_peer(5000, 16384)
    assert m.updates() == [5000]
    assert M.HpencModel(65536).updates() == [65536] and M.HpencModel(256).updates() == []


def test_bad_input_and_caps_commit_nothing():
    m = M.HpencModel()
    good = M.pack([(1, 0, [(b"x-a", b"1")]), (3, 1, [(b"x-b", b"2")])])
    w0, bw0, r0, _ = copy_of(m).encode(*good, 1 << 20, 8)
    for cap, bwc in ((len(w0) - 1, 8), (len(w0), 1)):
        w, bw, r, err = m.encode(*good, cap, bwc)
        assert (w, bw, err) == (b"", [], "capacity") and r == r0[:7] + (1,) and not m.table.entries and not m.stats["calls"]
    blocks, fields, arena = good
    for bad, code in ((([(1, 1, 2, 0)], fields, arena), M.ERR_FIELD_RANGE), (([(0, 0, 1, 0)], fields, arena), M.ERR_STREAM),
                      (([(1 << 31, 0, 1, 0)], fields, arena), M.ERR_STREAM),
                      (([(1, 0, 1, 0)], [(0, 3, 3, 1 << 24)], arena), M.ERR_LENGTH), (([(1, 0, 1, 0)], [(0, 7, 3, 2)], arena), M.ERR_STRING)):
        w, bw, r, err = m.encode(bad[0], bad[1], bad[2], 1 << 20, 8)
        assert err == "invalid" and r == (0, 0, 0, 0, 0, 0, M.BAD_INPUT | code << 8, 0) and not m.table.entries
    assert m.encode(*good, 1 << 20, 8)[:3] == (w0, bw0, r0)


def copy_of(m):
    import copy
    return copy.deepcopy(m)


# ---- the sweep of tests/test_zz_gpu_h2_hpenc_sweep.py: its witnesses, and its committed calls through both decoders ----------
PER_FAMILY = {"01": 28, "02": 20, "03": 40, "04": 15, "05": 12, "06": 10, "07": 87, "08": 43, "09": 11, "10": 44, "11": 14}


def test_every_case_of_the_hpenc_sweep_shows_its_witness():
    import collections
    from tests import h2_hpenc_sweep_lib as S
    cs = S.check_cases()
    assert collections.Counter(c["fam"] for c in cs) == PER_FAMILY and len(cs) == sum(PER_FAMILY.values()) == 324
    assert set(PER_FAMILY) == set(S.FAMILIES) and all(c["edge"] and c["key"] for c in cs)
    subset = S.emu_subset()
    assert {S.by_id(cid)["fam"] for cid in subset} == set(S.FAMILIES) and all(cid in subset for cid in S.CAUGHT_ALONE)
    assert all(S.links_cases(fam) for fam in S.FAMILIES)
    # the grid stride: calls of more occurrences than the stages have lanes, compared whole as every call is
    assert max(s["nocc"] for c in S.CASES if c["key"] == "grid" for s in S.simulate(c)) == 32769 > 2 * S.GRID
    assert max(s["nocc"] for c in S.links_cases("04") for s in S.simulate(c)) == 1025 > S.LINK_GRID
    # the ring is never full, and the sweep says so
    assert max(s["entries"] for c in S.CASES for s in S.simulate(c) if "entries" in s) == 1942 < M.RING
    assert not S.NGHTTP2_DIFFERS


def _pin(fam, make, resize, decode, table_of):
    """every committed call of the family's cases through a decoder that shares no code with the model: the header lists
    come back, and behind every call the decoder's dynamic table is the model's.  A ("peer", n) step is the decoder's side
    changing its SETTINGS_HEADER_TABLE_SIZE."""
    from tests import h2_hpenc_sweep_lib as S
    calls = 0
    for c in (c for c in S.CASES if c["fam"] == fam):
        dec, lead = make(c["table"])
        for item in S.pin_sequence(c):
            if item[0] == "peer":
                resize(dec, item[1])
                lead = b""
                continue
            _, lists, wire, table = item
            blocks = M.deframe(wire)
            assert [(s, es) for s, es, _ in blocks] == [(s, es) for s, es, _ in lists], c["id"]
            for (_, _, hs), (_, _, block) in zip(lists, blocks):
                got = decode(dec, lead + block)
                lead = b""
                assert got is not None, c["id"]
                assert [(n, v, h == 3) for n, v, h in hs] == [(n, v, r is True or r == 3) for n, v, r in got], c["id"]
            assert table_of(dec) == table, c["id"]
            calls += 1
    assert calls


@pytest.mark.parametrize("fam", sorted(PER_FAMILY))
def test_the_sweeps_calls_through_the_decoders_model(fam):
    _pin(fam, lambda n: (HpackTable(n), b""), lambda d, n: d.set_setting(n), lambda d, b: d.decode_block(b), lambda d: (d.entries, d.size))


@needs_nghttp2
@pytest.mark.parametrize("fam", sorted(PER_FAMILY))
def test_the_sweeps_calls_through_nghttp2(fam):
    """Both sides begin at 4096, or at the peer's table size where that is less, and no size update is sent for that
    (include/grdma_amd.h, "Header blocks, sending", 4; RFC 7541 Appendix C.6).  nghttp2's inflater can only be made at 4096
    and wants to be told of a smaller size in the first block it reads: the pin tells it, in front of the encoder's first
    block, what the encoder was created with.  Nothing else is added or left out; NGHTTP2_DIFFERS stays empty."""
    def make(n):
        return (L.Inflater(None if n == 4096 else n), M.enc_int(n, 5, 0x20) if n < 4096 else b"")

    _pin(fam, make, lambda d, n: d.change_table_size(n), lambda d, b: d.inflate(b), lambda d: d.table())
