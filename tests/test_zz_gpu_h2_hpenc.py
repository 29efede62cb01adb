"""Header blocks, sending: header lists in the decoder's layout encoded on the device into HEADERS and CONTINUATION frames
(grdma_h2_hpenc, csrc/grdma_h2_hpenc.h).  The expected values come from the HpencModel of tests/h2_hpenc_model.py: the
rules of include/grdma_amd.h ("Header blocks, sending").  Every comparison is exact (HE of tests/h2_hpenc_lib.py runs a
call on the device and in the model and compares the wire arena whole -- what is not written keeps its fill -- the
block-wire table, the result block, the table dump and the counters); what a test asserts beside that is what the case is
about.  One departure from the encoder's first specification ("a tie goes raw"): a string whose Huffman form is as long as its
raw bytes is sent CODED, because RFC 7541 Appendix C.6.2 (the authority on the bytes) codes "307" in three bytes."""
import json
import os

import pytest

from tests.h2_hpenc_lib import ERR2, FULL_COLLISION, HE, NAME_COLLISION, Wire, by_bits, chunk_lists, fill, huffman_bits
from tests.h2_hpenc_model import (BAD_INPUT, CHUNK, ERR_FIELD_RANGE, ERR_LENGTH, ERR_STREAM, ERR_STRING, HUFFMAN, deframe, enc_int, enc_str,
                                  pack)
from tests.h2_hpenc_sweep_lib import RAW, sized

pytestmark = pytest.mark.gpu

VECTORS = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "h2_hpenc_vectors.json")))


def block_of(h, fields, stream=1, flags=0):
    """one block of one call -> its bytes"""
    wire, bw, res = h.encode([(stream, flags, fields)])
    (s, es, block), = deframe(wire)
    assert (s, es) == (stream, flags & 1) and res[0] == 1
    return block


# ---- RFC 7541 Appendix C ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["C.4", "C.6"])
def test_the_rfcs_header_blocks(gpu, which):
    v = VECTORS[which]
    h = HE(gpu, v["table_size"])
    for k, b in enumerate(v["blocks"]):
        assert block_of(h, [(n.encode(), x.encode(), 1) for n, x in b["headers"]], 2 * k + 1) == bytes.fromhex(b["hex"])
        assert h.model.table.size == b["table_bytes"]
    h.close()


# ---- one field per block --------------------------------------------------------------------------------------------------------
def test_one_field_per_block(gpu):
    h = HE(gpu)
    wire, bw, res = h.encode([(1, 0, [(b":method", b"GET", 1)]),            # a static full match
                              (3, 0, [(b":path", b"/svc/M", 1)]),            # a static name match: inserted
                              (5, 0, [(b"x-new", b"value", 1)]),             # no match: a literal name, inserted
                              (7, 0, [(b"x-two", b"v", 2)]),                 # hint 2 without a match: not inserted
                              (9, 0, [(b"x-new", b"value", 2)]),             # hint 2 with a live full match: indexed
                              (11, 0, [(b"x-new", b"value", 3)]),            # hint 3 with a live full match: never indexed
                              (13, 0, [(b":method", b"GET", 3)])])
    blocks = [b for _, _, b in deframe(wire)]
    assert blocks[0] == b"\x82" and blocks[1] == b"\x44" + enc_str(b"/svc/M")
    assert blocks[2] == b"\x40" + enc_str(b"x-new") + enc_str(b"value") and blocks[3] == b"\x00" + enc_str(b"x-two") + enc_str(b"v")
    assert blocks[4] == b"\xbe" and blocks[5] == b"\x1f\x2f" + enc_str(b"value") and blocks[6] == b"\x12" + enc_str(b"GET")
    assert res[3:5] == (2, 0) and h.model.table.entries == [(b"x-new", b"value"), (b":path", b"/svc/M")]
    h.close()


# ---- prefix edges -----------------------------------------------------------------------------------------------------------------
def test_indexed_fields_at_126_127_128(gpu):
    h = HE(gpu)
    fs = fill(70)
    h.encode([(1, 0, fs)])
    # entry i stands at index 62 + 69 - i
    assert block_of(h, [fs[5], fs[4], fs[3]]) == b"\xfe" + b"\xff\x00" + b"\xff\x01"
    h.close()


@pytest.mark.parametrize("idx", [62, 63, 64])
def test_a_name_index_on_the_six_bit_prefix(gpu, idx):
    h = HE(gpu)
    fs = fill(3)
    h.encode([(1, 0, fs)])
    assert block_of(h, [(fs[64 - idx][0], b"other", 1)]) == enc_int(idx, 6, 0x40) + enc_str(b"other")
    assert block_of(h, [(fs[64 - idx][0], b"third", 1)])[0] == 0x40 | 62  # (the newest entry of that name is the last one's)
    h.close()


def test_name_indices_on_the_four_bit_prefix(gpu):
    # (14 cannot be a name reference: the static entries 8..14 share the name :status, and the lowest index is taken)
    h = HE(gpu)
    fs = fill(3)
    h.encode([(1, 0, fs)])
    b = block_of(h, [(b":status", b"599", 2), (b"accept-charset", b"x", 2), (b"accept-encoding", b"x", 3), (fs[2][0], b"o", 2),
                     (fs[1][0], b"o", 3), (fs[0][0], b"o", 2)])
    assert b == (b"\x08" + enc_str(b"599") + b"\x0f\x00" + enc_str(b"x") + b"\x1f\x01" + enc_str(b"x") + b"\x0f\x2f" + enc_str(b"o") +
                 b"\x1f\x30" + enc_str(b"o") + b"\x0f\x31" + enc_str(b"o"))
    h.close()


def test_string_lengths_at_126_127_128(gpu):
    h = HE(gpu)
    b = block_of(h, [(b"x-l", RAW * n, 2) for n in (126, 127, 128)] + [(b"x-l", b"a" * n, 2) for n in (201, 203, 204)])
    name = b"\x00" + enc_str(b"x-l")
    assert b == (name + b"\x7e" + RAW * 126 + name + b"\x7f\x00" + RAW * 127 + name + b"\x7f\x01" + RAW * 128 +
                 name + enc_str(b"a" * 201) + name + enc_str(b"a" * 203) + name + enc_str(b"a" * 204))
    assert [enc_str(b"a" * n)[:2] for n in (201, 203, 204)] == [b"\xfe\x18", b"\xff\x00", b"\xff\x01"]
    h.close()


# ---- Huffman ------------------------------------------------------------------------------------------------------------------------
def test_every_byte_value_as_a_one_byte_string(gpu):
    h = HE(gpu)
    b = block_of(h, [(b"x-b", bytes([s]), 2) for s in range(256)])
    name = b"\x00" + enc_str(b"x-b")
    assert b == b"".join(name + (bytes([0x81, HUFFMAN[s][0] << (8 - HUFFMAN[s][1]) | 0xff >> HUFFMAN[s][1]]) if HUFFMAN[s][1] <= 8
                                 else bytes([0x01, s])) for s in range(256))
    h.close()


def test_huffman_only_where_it_is_not_longer(gpu):
    h = HE(gpu)
    thirty = bytes([by_bits(30)])
    assert huffman_bits(thirty) == 30
    run = bytes(s for s in range(256) if HUFFMAN[s][1] == 30)[:3] + b"a" * 24   # 210 bits: 27 bytes, as long as raw
    cases = [b"307",                 # 17 bits: three bytes, as long as raw -> coded (RFC 7541 C.6.2)
             b"30",                  # 11 bits: two bytes, as long as raw -> coded
             b"www",                 # 21 bits: one byte less -> coded
             b"\x00",                # 13 bits: one byte more -> raw
             b"a" * 7 + b"\x00",     # 48 bits: six bytes
             (thirty + b"a" * 8) * 4,  # 30-bit symbols between short ones
             run, b"",
             thirty * 5]             # a run of 30-bit symbols alone: raw
    b = block_of(h, [(b"x-h", v, 2) for v in cases])
    assert b == b"".join(b"\x00" + enc_str(b"x-h") + enc_str(v) for v in cases)
    assert [bool(enc_str(v)[0] & 0x80) for v in cases] == [True, True, True, False, True, True, True, False, False]
    assert len(enc_str(run)) == 1 + len(run)
    h.close()


def test_every_bit_alignment_of_the_padding(gpu):
    h = HE(gpu)
    vals = [b"a" * k for k in range(1, 9)] + [b"-" * k for k in range(1, 5)]  # 5 k and 6 k bits
    assert {huffman_bits(v) % 8 for v in vals} == set(range(8))
    b = block_of(h, [(v + b"n", v, 2) for v in vals])  # (names are coded by the same rule)
    assert b == b"".join(b"\x00" + enc_str(v + b"n") + enc_str(v) for v in vals)
    h.close()


# ---- the dynamic table --------------------------------------------------------------------------------------------------------------
def test_the_same_field_twice_in_a_block_across_blocks_and_across_calls(gpu):
    h = HE(gpu)
    f = (b"x-twice", b"value", 1)
    wire, _, res = h.encode([(1, 0, [f, f]), (3, 0, [f])])
    assert [b for _, _, b in deframe(wire)] == [b"\x40" + enc_str(b"x-twice") + enc_str(b"value") + b"\xbe", b"\xbe"] and res[3] == 1
    assert block_of(h, [f, (b"x-twice", b"other", 1), f]) == b"\xbe" + b"\x7e" + enc_str(b"other") + b"\xbf"
    h.close()


def test_an_insertion_evicts_what_a_later_field_had_matched(gpu):
    h = HE(gpu, 100)  # room for two entries of 36 bytes
    a, b, c = (b"x-a", b"1", 1), (b"x-b", b"2", 1), (b"x-c", b"3", 1)
    h.encode([(1, 0, [a, b])])
    # c evicts a, which the second field had matched in front of the step: a literal again, inserted again (b goes)
    assert block_of(h, [c, a]) == b"\x40" + enc_str(b"x-c") + enc_str(b"3") + b"\x40" + enc_str(b"x-a") + enc_str(b"1")
    assert h.model.table.entries == [(b"x-a", b"1"), (b"x-c", b"3")]
    # ... and a name match that goes: d evicts c, whose name the second field had found
    assert block_of(h, [(b"x-d", b"4", 1), (b"x-c", b"9", 2)]) == b"\x40" + enc_str(b"x-d") + enc_str(b"4") + b"\x00" + enc_str(b"x-c") + enc_str(b"9")
    # an entry matched that stays: its index moves with the insertion in front of it
    assert block_of(h, [(b"x-e", b"5", 1), (b"x-d", b"4", 1)]) == b"\x40" + enc_str(b"x-e") + enc_str(b"5") + b"\xbf"
    h.close()


def test_entries_of_exactly_the_table_size_one_more_and_size_zero(gpu):
    h = HE(gpu, 100)
    h.encode([(1, 0, [(b"x-a", b"1", 1)])])
    block_of(h, [(b"n" * 34, b"v" * 34, 1)])   # 100 bytes: it alone stays
    assert h.model.table.entries == [(b"n" * 34, b"v" * 34)] and h.model.table.size == 100
    b = block_of(h, [(b"n" * 34, b"v" * 35, 1), (b"n" * 34, b"v" * 34, 1)])  # 101: the table empties, nothing is inserted
    assert b[0] == 0x7e and h.model.table.entries == [(b"n" * 34, b"v" * 34)]  # (the name reference stood in front of the evictions)
    assert b[1 + len(enc_str(b"v" * 35))] == 0x40
    h.close()
    h = HE(gpu, 0)
    f = (b"x-a", b"1", 1)
    assert block_of(h, [f, f]) == (b"\x40" + enc_str(b"x-a") + enc_str(b"1")) * 2 and not h.model.table.entries
    h.close()


def test_the_ring_at_its_most_entries(gpu):
    h = HE(gpu, 65536)
    fs = [(bytes([0x61 + i // 256]), bytes([i % 256]), 1) for i in range(2000)]  # 34 bytes an entry: 1927 live
    wire, _, res = h.encode([(1, 0, fs)])
    assert wire[9:13] == b"\x3f\xe1\xff\x03" and res[3:6] == (2000, 73, 1927 * 34)
    oldest, newest = fs[73], fs[1999]
    # (the evicted field's name lives on in the entries 73..255: the newest of them is 1743 entries back)
    assert block_of(h, [oldest, newest, fs[72]]) == enc_int(62 + 1926, 7, 0x80) + b"\xbe" + enc_int(62 + 1999 - 255, 6, 0x40) + enc_str(fs[72][1])
    h.close()


def test_the_byte_ring_across_its_wrap(gpu):
    h = HE(gpu, 65536)
    h.encode([(1, 0, [(b"x-0", b"zero", 1)])])  # (the size update is out)
    sent = []
    for call in range(7):  # 7 x 10 x 1003 string bytes: the ring's head passes 65536
        fs = [(b"x-w", bytes([0x30 + call, 0x30 + k]) * 500, 1) for k in range(10)]
        sent += fs
        h.encode([(1, 0, fs)])
    live = h.model.table.entries
    assert len(live) == 63 and sum(len(n) + len(v) for n, v, _ in sent) > 65536
    b = block_of(h, [(n, v, 2) for n, v in live])  # every live entry is found in the ring, the one across the wrap too
    assert b == b"".join(enc_int(62 + i, 7, 0x80) for i in range(63))
    h.close()


# ---- hash collisions ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [0, 1])
def test_equal_hashes_never_decide(gpu, order):
    (n1, v1), (n2, v2) = FULL_COLLISION[::1 - 2 * order]
    a, b = NAME_COLLISION[::1 - 2 * order]
    h = HE(gpu)
    h.encode([(1, 0, [(n1, v1, 1), (a, b"v", 1)])])
    # against the table in front of the step: the other field of the pair is no full match, the other name no name match
    blk = block_of(h, [(n2, v2, 2), (b, b"v", 2), (n1, v1, 2), (a, b"v", 2)])
    assert blk == b"\x0f\x30" + enc_str(v2) + b"\x00" + enc_str(b) + enc_str(b"v") + b"\xbf\xbe"
    h.close()
    # ... and against an entry of the same step (the patch behind an insertion)
    h = HE(gpu)
    blk = block_of(h, [(n1, v1, 1), (n2, v2, 1), (a, b"v", 1), (b, b"v", 1)])
    assert blk == (b"\x40" + enc_str(n1) + enc_str(v1) + b"\x7e" + enc_str(v2) + b"\x40" + enc_str(a) + enc_str(b"v") +
                   b"\x40" + enc_str(b) + enc_str(b"v"))
    h.close()


# ---- the walk's steps -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [CHUNK - 1, CHUNK, CHUNK + 1])
def test_fields_per_block_around_a_step(gpu, n):
    h = HE(gpu)
    wire, bw, res = h.encode(chunk_lists(n))
    assert res[:2] == (1, 1) and res[3] == 0
    h.close()


@pytest.mark.parametrize("slot", [CHUNK, CHUNK - 1], ids=["first", "last"])
def test_the_inserting_field_in_a_steps_first_and_last_slot(gpu, slot):
    h = HE(gpu)
    fs = [(n, v, 2) for n, v in fill(CHUNK + 40)]
    ins = (b"x-ins", b"here", 1)
    fs[slot] = ins
    fs[slot + 1] = fs[CHUNK + 30] = ins  # found through the patch, or in the table in front of the next step
    fs[slot + 2] = (b"x-ins", b"other", 2)
    wire, _, res = h.encode([(1, 0, fs[:100]), (3, 0, fs[100:])])
    assert res[3] == 1 and wire.count(b"\xbe") >= 2
    h.close()


def test_three_hundred_blocks_an_empty_block_and_zero_blocks(gpu):
    h = HE(gpu)
    lists = [(2 * k + 1, k & 1, [(b":status", b"200", 1), (b"content-type", b"application/grpc", 1), (b"x-k", b"%d" % (k % 7), 1)])
             for k in range(300)]
    lists[150] = (301, 1, [])
    wire, bw, res = h.encode(lists)
    assert res[:2] == (300, 300) and bw[150][1:] == (9, 1) and wire[bw[150][0]:bw[150][0] + 9] == bytes.fromhex("000000010500") + b"\x00\x01\x2d"
    assert h.encode([])[2][:3] == (0, 0, 0)
    h.set_peer(100)
    assert h.encode([])[2][:3] == (0, 0, 0)   # (no block: the size update waits)
    assert block_of(h, [])[:2] == b"\x3f\x45"  # an empty block, but the call's first: it carries the update
    h.close()


def test_a_run_of_empty_blocks_longer_than_a_step(gpu):
    # (the walk stages the places of 257 blocks a step: the field behind 300 empty blocks finds its block behind them)
    h = HE(gpu)
    f = (b"x-e", b"1", 1)
    wire, bw, res = h.encode([(1, 0, [f])] + [(2 * k + 3, 0, []) for k in range(300)] + [(999, 1, [f, f])] + [(1001, 0, [])] * 2)
    assert res[:2] == (304, 304) and bw[301] == (bw[300][0] + 9, 11, 1) and wire[bw[301][0]:bw[301][0] + 11] == bytes.fromhex("0000020105000003e7bebe")
    h.close()


# ---- frames ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("length", [16384, 16385, 2 * 16384 + 1])
def test_blocks_around_the_max_frame_size(gpu, length):
    h = HE(gpu)
    wire, bw, res = h.encode([(2 ** 31 - 1, 1, sized(length)), (3, 0, [(b":method", b"GET")])])
    nfr = (length + 16383) // 16384
    assert res[:2] == (2, nfr + 1) and bw[0] == (0, length + 9 * nfr, nfr) and bw[1] == (length + 9 * nfr, 10, 1)
    assert wire[:9] == b"\x00\x40\x00\x01" + (b"\x05" if nfr == 1 else b"\x01") + b"\x7f\xff\xff\xff"
    if nfr > 1:
        last = 9 * (nfr - 1) + 16384 * (nfr - 1)
        assert wire[last:last + 9] == b"\x00\x00\x01\x09\x04\x7f\xff\xff\xff"
    h.close()


def test_fields_cut_by_a_frame_inside_an_integer_and_inside_a_huffman_body(gpu):
    h = HE(gpu)
    # the second field: 00, the name (4 bytes), the value's length in 3 bytes from byte 5 on: the cut falls behind its first
    wire, bw, res = h.encode([(1, 0, sized(16384 - 6, [(b"x-f", RAW * 300, 2)]))])
    assert res[1] == 2 and wire[9 + 16383] == 0x7f and wire[9 + 16384:9 + 16384 + 9] == (300 + 8 - 6).to_bytes(3, "big") + b"\x09\x04\x00\x00\x00\x01"
    # a Huffman body of 63 bytes from byte 6 on, the cut 30 bytes into it
    wire, bw, res = h.encode([(1, 0, sized(16384 - 36, [(b"x-f", b"a" * 100, 2)]))])
    body = enc_str(b"a" * 100)[1:]
    assert res[1] == 2 and wire[9 + 16384 - 30:9 + 16384] == body[:30] and wire[18 + 16384:18 + 16384 + 33] == body[30:]
    # an indexed field of two bytes across the cut
    fs = fill(70)
    h.encode([(1, 0, fs)])
    wire, bw, res = h.encode([(1, 0, sized(16384 - 1, [fs[3]]))])
    assert res[1] == 2 and wire[9 + 16383] == 0xff and wire[18 + 16384] == 0x01
    h.close()


def test_the_max_frame_size_changed_by_set_peer(gpu):
    h = HE(gpu)
    assert h.encode([(1, 0, sized(20001))])[2][1] == 2
    h.set_peer(4096, 20000)
    wire, bw, res = h.encode([(1, 0, sized(20001))])
    assert res[1] == 2 and wire[:3] == (20000).to_bytes(3, "big") and bw[0] == (0, 20001 + 18, 2)
    h.set_peer(4096, 2 ** 24 - 1)
    assert h.encode([(1, 0, sized(20001))])[2][1] == 1
    h.close()


# ---- size updates ---------------------------------------------------------------------------------------------------------------------
def test_size_updates_between_calls(gpu):
    h = HE(gpu)
    h.encode([(1, 0, fill(20))])
    h.set_peer(100)  # lowered: one update, the evictions first
    b = block_of(h, [fill(20)[19], fill(20)[0]])
    assert b[:2] == b"\x3f\x45" and b[2] == 0xbe and b[3] == 0x40 and h.model.table.max_size == 100
    h.set_peer(50)
    h.set_peer(200)  # lowered, then raised: two
    wire, _, res = h.encode([(1, 0, [fill(20)[19]]), (3, 0, [fill(20)[19]])])  # (50 bytes keep the newest entry alone)
    blocks = [x for _, _, x in deframe(wire)]
    assert blocks[0][:5] == b"\x3f\x13\x3f\xa9\x01" and blocks[0][5] == 0x40 and blocks[1] == b"\xbe" and res[4] == 1
    h.set_peer(0)
    h.set_peer(200)  # to 0 and back: the table is emptied on both sides
    assert block_of(h, [fill(20)[0]])[:5] == b"\x20\x3f\xa9\x01\x40"
    assert block_of(h, [fill(20)[0]]) == b"\xbe"
    h.close()
    h = HE(gpu, 65536)  # a peer that announced more than 4096: the first block says so
    assert block_of(h, [(b":method", b"GET")]) == b"\x3f\xe1\xff\x03\x82"
    h.close()


# ---- caps -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("short", ["wire", "block-wire"])
def test_a_cap_too_small_commits_nothing_and_the_repeat_is_exact(gpu, short):
    lists = [(1, 0, fill(5)), (3, 1, fill(8)), (5, 0, fill(3))]
    ref = HE(gpu)
    ref.encode([(1, 0, fill(2))])
    ref.set_peer(300)
    want = ref.encode(lists)
    h = HE(gpu)
    h.encode([(1, 0, fill(2))])
    h.set_peer(300)
    before = h.enc.table()
    got = h.encode(lists, **({"wire_cap": want[2][2] - 1} if short == "wire" else {"bw_cap": 2}))
    assert got[2] == want[2][:7] + (1,) and h.enc.table() == before
    assert h.encode(lists) == want  # (the size update was not taken either)
    h.close()
    ref.close()


# ---- bad input --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["range", "string", "stream0", "stream31", "length"])
def test_bad_input_in_the_third_block_of_five(gpu, kind):
    lists = [(2 * k + 1, 0, fill(3, b"b%d" % k)) for k in range(5)]
    blocks, fields, arena = pack(lists)
    blocks, fields = list(blocks), list(fields)
    no, vo, nl, vl = fields[7]
    if kind == "range":
        blocks[2] = (5, 13, 3, 0)
    elif kind == "string":
        fields[7] = (no, len(arena) - 3, nl, 4)
    elif kind == "stream0":
        blocks[2] = (0, 6, 3, 0)
    elif kind == "stream31":
        blocks[2] = (1 << 31, 6, 3, 0)
    else:
        fields[7] = (no, vo, nl, 1 << 24)
    code = {"range": ERR_FIELD_RANGE, "string": ERR_STRING, "length": ERR_LENGTH}.get(kind, ERR_STREAM)
    h = HE(gpu)
    h.encode([(1, 0, fill(2))])
    wire, bw, res = h.encode(raw=(blocks, fields, arena), wire_cap=4096, bw_cap=8)
    assert res == (0, 0, 0, 0, 0, h.model.table.size, BAD_INPUT | code << 8 | 2 << 32, 0) and wire == b"" and len(h.model.table.entries) == 2
    assert h.encode(lists)[2][:2] == (5, 5)  # not sticky: the next good call is exact
    h.close()


# ---- end to end on the device -----------------------------------------------------------------------------------------------------------
def test_decoder_output_forwards_unchanged(gpu):
    from tests.h2_helpers import grpcio_capture
    from tests.h2_hpack_lib import HH
    capture, _ = grpcio_capture()
    a = HH(gpu, prefix=True)
    a.deframe([capture])
    lists, res = a.decode()
    t = a.target
    raw = tuple(x.read() for x in (t.blocks, t.fields, t.strings))
    words = lambda data, n: [tuple(int.from_bytes(data[16 * i + 4 * j:16 * i + 4 * j + 4], "little") for j in range(4)) for i in range(n)]  # noqa: E731
    e = HE(gpu)
    # the decoder's three device targets, unchanged, are the encoder's input
    wire, bw, eres = e.encode(raw=(words(raw[0], res[0]), words(raw[1], res[1]), raw[2][:res[2]]),
                              device=(t.blocks.ptr, res[0], t.fields.ptr, res[1], t.strings.ptr, res[2]))
    assert eres[0] == 5 and [s for s, _, _ in deframe(wire)] == [1, 3, 5, 7, 9]
    b = HH(gpu)
    again, _ = b.feed([wire])
    assert again == lists
    assert b.dec.table()[0] == e.enc.table()[0] and b.dec.table()[1][:2] == e.enc.table()[1][:2]
    for x in (a, b, e):
        x.close()


# ---- refusals and lifetime ----------------------------------------------------------------------------------------------------------------
def test_refusals_and_lifetime(gpu):
    from grpc_rdma_amd import h2dev
    for args in ((65537, 16384), (4096, 16383), (4096, 1 << 24)):
        with pytest.raises(gpu.GrdmaError):
            h2dev.HeaderEncoder(*args)
    h = HE(gpu)
    for args in ((65537, 16384), (4096, 16383), (4096, 1 << 24)):
        with pytest.raises(gpu.GrdmaError, match=ERR2):
            h.enc.set_peer(*args)
    w = Wire(gpu, 256, 4)
    wp, wc, bp, bc = w.args()
    for targets in ((0, wc, bp, bc), (wp, 0, bp, bc), (wp, wc, 0, bc), (wp, wc, bp, 0), (wp + 8, wc, bp, bc), (wp, wc, bp + 8, bc)):
        with pytest.raises(gpu.GrdmaError, match=ERR2):
            h.enc.encode(0, 0, 0, 0, 0, 0, *targets)
    with pytest.raises(gpu.GrdmaError, match=ERR2):
        h.enc.encode(0, 1, 0, 0, 0, 0, wp, wc, bp, bc)  # a count without a table
    assert w.wire.read() == bytes([0xA5]) * (256 + 64)
    h.encode([(1, 0, fill(2))])  # nothing of that changed anything
    h.close()
    h.close()
    with pytest.raises(gpu.GrdmaError, match=ERR2):
        h.enc.encode(0, 0, 0, 0, 0, 0, wp, wc, bp, bc)
    for _ in range(3):  # create and destroy with a call in between
        x = HE(gpu, 256)
        x.encode([(1, 0, fill(4))])
        x.close()
