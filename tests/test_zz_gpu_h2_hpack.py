"""Header blocks on the device: the HPACK blocks of a deframing's HEADERS and CONTINUATION frames decoded into a block
table, a field table and a string arena (grdma_h2_hpack, csrc/grdma_h2_hpack.h).  The expected values come from the
HpackModel of tests/h2_hpack_model.py: the rules of include/grdma_amd.h ("Header blocks") applied to the ORACLE's event
list and the bytes fed.  Every comparison is exact (HH of tests/h2_hpack_lib.py runs a call on the device and in the
model and compares the three targets whole -- what is not written keeps its fill -- the result block, the dynamic table
and the counters); what a test asserts beside that is what the case is about."""
import pytest

from tests.h2_control_lib import bad_flags, data, ping, settings
from tests.h2_device_lib import same
from tests.h2_helpers import frame, grpcio_capture
from tests.h2_hpack_lib import ERR5, HH, Targets, capture_blocks, enc_int, headers_frames, huff, indexed, literal, size_update
from tests.h2_hpack_model import (ERR_BLOCK_TOO_LARGE, ERR_DEFRAMER, ERR_HUFFMAN, ERR_INDEX, ERR_INTEGER, ERR_PADDING, ERR_SIZE_UPDATE,
                                  ERR_TRUNCATED, FAILED, HUFFMAN, LOST, OPEN, STATIC)

pytestmark = pytest.mark.gpu

NINE = bytes.fromhex("c4c38386c2c1c0bfbe")  # the capture's fully indexed block


def word(flags, err=0, stream=0):
    return flags | err << 8 | stream << 32


def one(h, block, sid=1, **kw):
    """one block in frames of its own through a deframing and a decode -> (its fields, result)"""
    blocks, res = h.feed([headers_frames(sid, block, **kw)])
    return (blocks[0][2] if blocks else None), res


def failing(h, block, err, sid=1):
    fields, res = one(h, block, sid)
    assert fields is None and res == (0, 0, 0, 0, 0, h.model.table.size, word(FAILED, err, sid), 0)
    # sticky: the next call is taken, writes nothing and says the same
    assert h.feed([headers_frames(sid + 2, b"\x82")])[1][6:] == (word(FAILED, err, sid), 0)


# ---- the capture and cuts -------------------------------------------------------------------------------------------------
def test_the_grpcio_capture_whole(gpu):
    capture, _ = grpcio_capture()
    h = HH(gpu, prefix=True)
    blocks, res = h.feed([capture])
    assert res[:3] == (5, 45, sum(len(n) + len(v) for _, _, fs in blocks for n, v, _ in fs)) and res[6:] == (0, 0)
    assert [s for s, _, _ in blocks] == [1, 3, 5, 7, 9] and all(len(fs) == 9 for _, _, fs in blocks)
    assert blocks[0][2][0][0] == b":path" and blocks[0][2][0][2] == 1
    assert dict((n, v) for n, v, _ in blocks[4][2])[b":path"] == b"/mb.BenchmarkService/ClientStream"
    assert h.model.table.entries[0][0] == b"grpc-timeout"
    h.close()


def test_the_capture_in_one_byte_slices(gpu):
    capture, _ = grpcio_capture()
    part = capture[:529]  # the preface, SETTINGS and the first three requests' HEADERS
    h = HH(gpu, prefix=True)
    blocks, res = h.feed([part[i:i + 1] for i in range(len(part))])
    assert res[:2] == (3, 27) and [s for s, _, _ in blocks] == [1, 3, 5]
    h.close()


# the first HEADERS frame of the capture: header at 91, 234 payload bytes from 100 on.  Its block begins 40 (literal with
# incremental indexing, new name) 05 ":path" 1e ... : byte 1 is a string's length, bytes 2.. the string
@pytest.mark.parametrize("cut", [95, 100, 101, 102, 104, 109, 120, 333], ids=lambda c: "at%d" % c)
def test_the_capture_cut_between_calls(gpu, cut):
    # inside the frame header, after 0 and 1 payload bytes, behind a string's length, inside the name, behind it (inside
    # the field: in front of the value's length), inside the value, one byte short of the block's end
    capture, _ = grpcio_capture()
    part = capture[:529]
    h = HH(gpu, prefix=True)
    a = h.feed([part[:cut]])[1]
    assert a[0] == 0 and a[6] == (OPEN if cut >= 100 else 0)  # (the FRAME event opens the block)
    blocks, res = h.feed([part[cut:]])
    assert res[:2] == (3, 27) and res[6] == 0 and blocks[0][0] == 1
    h.close()


def test_a_block_with_long_integers_cut_at_every_byte(gpu):
    # non-minimal indices, a two-byte string length, a Huffman string: every cut of the frame's payload and header
    block = indexed(2) + literal(b"x-long", b"v" * 130) + literal(16, b"gzip", mode=2, extra=2) + literal(62, b"www.example.com", mode=3, hv=True)
    wire = headers_frames(1, block, flags=1)
    for cut in list(range(1, 24)) + [len(wire) - 40, len(wire) - 1]:
        h = HH(gpu)
        assert h.feed([wire[:cut]])[1][0] == 0
        blocks, res = h.feed([wire[cut:]])
        assert res[:2] == (1, 4) and blocks[0][:2] == (1, 1), cut
        h.close()


# ---- frame shapes ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pad", [0, 3])
def test_padded_and_prioritised(gpu, pad):
    h = HH(gpu)
    wire = headers_frames(1, NINE[2:4] + literal(b"a", b"b"), flags=1, pad=pad, priority=True, cont=(1,))
    blocks, res = h.feed([wire])
    assert blocks == [(1, 3, [STATIC[3] + (0,), STATIC[6] + (0,), (b"a", b"b", 1)])] and res[:3] == (1, 3, 24)
    # ... and cut inside the priority bytes and inside the padding
    for cut in (9 + 3, 17 if pad else 15):
        h2 = HH(gpu)
        h2.feed([wire[:cut]])
        assert h2.feed([wire[cut:]])[0] == blocks
        h2.close()
    h.close()


@pytest.mark.parametrize("case", ["too short", "pad length"])
def test_padding_errors(gpu, case):
    h = HH(gpu)
    good = headers_frames(1, b"\x82")
    if case == "too short":   # PADDED | PRIORITY with 5 payload bytes: one short of the pad length and the priority
        bad = frame(1, 4 | 8 | 0x20, 3, bytes(5))
    else:                     # the pad length covers everything that is left
        bad = frame(1, 4 | 8, 3, bytes([2]) + b"\x82" + bytes(1))
    blocks, res = h.feed([good + bad + headers_frames(5, b"\x82")])
    assert [b[0] for b in blocks] == [1] and res[6] == word(FAILED, ERR_PADDING, 3)
    assert h.feed([good])[1] == (0, 0, 0, 0, 0, 0, word(FAILED, ERR_PADDING, 3), 0)
    h.close()


def test_continuations_with_a_call_boundary_inside_the_second(gpu):
    block = literal(b"name-one", b"value-one") + literal(b"name-two", b"v" * 40, hv=True) + indexed(62) + indexed(63)
    wire = headers_frames(7, block, cont=(5, 20, 41))
    h = HH(gpu)
    at = 9 + 5 + 9 + 15 + 9 + 10  # ten bytes into the second CONTINUATION
    assert h.feed([wire[:at]])[1][6] == OPEN
    blocks, res = h.feed([wire[at:]])
    assert res[:2] == (1, 4) and [f[0] for f in blocks[0][2]] == [b"name-one", b"name-two", b"name-two", b"name-one"]
    # between two frames of a block: the call ends behind the HEADERS frame's last byte
    wire = headers_frames(9, indexed(62) + indexed(2), cont=(1,))
    assert h.feed([wire[:10]])[1][6] == OPEN
    assert h.feed([wire[10:]])[0] == [(9, 0, [(b"name-two", b"v" * 40, 0), STATIC[2] + (0,)])]
    h.close()


def test_data_of_other_streams_between_blocks_and_a_refused_stream(gpu):
    h = HH(gpu, streams=(1, 3))
    wire = (headers_frames(1, literal(b"k", b"1")) + data(3, b"x" * 300) + ping(7) + headers_frames(3, indexed(62), flags=1) +
            data(1, b"y" * 20) + headers_frames(44, indexed(62) + literal(b"k", b"2")) + settings(1) + headers_frames(1, indexed(62)))
    blocks, res = h.feed([wire])
    # (stream 44 is not in the client parser's map: its block is decoded all the same, and the table follows)
    assert [(s, fl, [f[:2] for f in fs]) for s, fl, fs in blocks] == [
        (1, 0, [(b"k", b"1")]), (3, 1, [(b"k", b"1")]), (44, 0, [(b"k", b"1"), (b"k", b"2")]), (1, 0, [(b"k", b"2")])]
    h.close()


# ---- many blocks -----------------------------------------------------------------------------------------------------------
def test_three_hundred_indexed_blocks_with_inserting_blocks_among_them(gpu):
    first = capture_blocks()[0][1]
    wire = bytearray(headers_frames(1, first))
    sid = 3
    for k in range(300):
        if k == 150:  # an inserting block in the middle: what was 62 is 63 from here on
            wire += headers_frames(sid, literal(b"grpc-timeout", b"2S", hv=True) + NINE[:8] + indexed(62))
            sid += 2
        wire += headers_frames(sid, NINE if k < 150 else bytes([0xc5, 0xc4, 0x83, 0x86, 0xc3, 0xc2, 0xc1, 0xc0, 0xbf]))
        sid += 2
    h = HH(gpu, caps=(512, 4096, 1 << 17))
    blocks, res = h.feed([bytes(wire)])
    assert res[:2] == (302, 9 * 301 + 10) and res[6:] == (0, 0)
    assert blocks[150][2] == blocks[1][2] and blocks[152][2] == blocks[1][2] and blocks[151][2][0][:2] == (b"grpc-timeout", b"2S")
    h.close()


def test_references_to_entries_inserted_in_this_block_the_previous_block_and_the_previous_call(gpu):
    h = HH(gpu)
    a = literal(b"alpha", b"1") + indexed(62) + literal(62, b"2") + literal(62, b"3") + literal(62, b"4") + indexed(62)
    b = indexed(62) + indexed(65) + literal(63, b"5", mode=3)
    blocks, res = h.feed([headers_frames(1, a) + headers_frames(3, b)])
    # (a chain of three name references: each literal names the entry the one before it inserted)
    assert [f[:2] for f in blocks[0][2]] == [(b"alpha", b"1"), (b"alpha", b"1"), (b"alpha", b"2"), (b"alpha", b"3"), (b"alpha", b"4"), (b"alpha", b"4")]
    assert [f[:2] for f in blocks[1][2]] == [(b"alpha", b"4"), (b"alpha", b"1"), (b"alpha", b"5")] and res[3] == 4
    blocks, res = h.feed([headers_frames(5, indexed(62) + indexed(65) + literal(64, b"6") + indexed(62))])
    assert [f[:2] for f in blocks[0][2]] == [(b"alpha", b"4"), (b"alpha", b"1"), (b"alpha", b"6"), (b"alpha", b"6")]
    h.close()


# ---- prefix edges ----------------------------------------------------------------------------------------------------------
def test_index_and_length_prefix_edges(gpu):
    h = HH(gpu)
    fill = b"".join(literal(b"n%d" % k, b"v%d" % k) for k in range(3))  # entries 62, 63, 64: n2, n1, n0
    block = fill + indexed(61) + indexed(62) + indexed(63) + indexed(64) + literal(14, b"a", mode=2) + literal(15, b"b", mode=2) + \
        literal(16, b"c", mode=3) + literal(62, b"d") + literal(63 + 1, b"e") + b"".join(literal(b"s", b"z" * n, mode=2) for n in (0, 126, 127, 128))
    fields, res = one(h, block)
    assert [f[0] for f in fields[3:11]] == [STATIC[61][0], b"n2", b"n1", b"n0", STATIC[14][0], STATIC[15][0], STATIC[16][0], b"n2"]
    assert [len(f[1]) for f in fields[-4:]] == [0, 126, 127, 128]
    # ... the same lengths as Huffman strings: 126 and 127 raw bytes of code
    fields, res = one(h, b"".join(literal(b"s", b"0" * n, mode=2, hv=True) for n in (0, 201, 203, 204)), sid=3)
    assert [len(f[1]) for f in fields] == [0, 201, 203, 204]
    h.close()


# ---- Huffman ---------------------------------------------------------------------------------------------------------------
def test_huffman_all_byte_values_and_seven_bits_of_padding(gpu):
    h = HH(gpu)
    every = bytes(range(256))
    fields, res = one(h, literal(every[::-1], every, hn=True, hv=True))
    assert fields == [(every[::-1], every, 1)]
    seven = b"00000"  # five codes of five bits: 25 bits and 7 of padding
    assert HUFFMAN[ord("0")][1] == 5
    assert one(h, literal(b"p", seven, hv=True), sid=3)[0] == [(b"p", seven, 1)]
    h.close()


@pytest.mark.parametrize("case", ["eos", "eight bits of padding", "a zero bit in the padding"])
def test_huffman_errors(gpu, case):
    h = HH(gpu)
    if case == "eos":
        body = (0x3fffffff << 2 | 3).to_bytes(4, "big")  # EOS and two bits of padding
    elif case == "eight bits of padding":
        body = huff(b"00000000", pad_bits=8)  # (eight codes of five bits end on a byte)
    else:
        body = huff(b"0", pad_bits=3, pad_ones=False)
    failing(h, b"\x00\x01k" + enc_int(len(body), 7, 0x80) + body, ERR_HUFFMAN)
    h.close()


# ---- the dynamic table -----------------------------------------------------------------------------------------------------
def test_a_table_filled_to_the_byte_then_one_byte_more(gpu):
    h = HH(gpu)
    # 4096 = 63 entries of 64 bytes (32 + 2 + 30) and one of 64 with another name: exactly full
    block = b"".join(literal(b"%02d" % k, b"v" * 30) for k in range(64))
    fields, res = one(h, block)
    assert res[3:6] == (64, 0, 4096) and len(h.model.table.entries) == 64
    fields, res = one(h, literal(b"n", b""), sid=3)  # 33 bytes: one entry goes
    assert res[3:6] == (1, 1, 4096 - 64 + 33)
    fields, res = one(h, literal(b"n", b"w" * 32), sid=5)  # 65 bytes into 31 free: one more goes
    assert res[3:6] == (1, 1, 4096 - 128 + 33 + 65)
    h.close()


def test_an_entry_larger_than_the_table_and_size_updates(gpu):
    h = HH(gpu, setting=256)
    fields, res = one(h, literal(b"a", b"1") + literal(b"b", b"x" * 300) + literal(b"c", b"3"))
    assert res[3:6] == (2, 1, 34) and [f[:2] for f in fields][1] == (b"b", b"x" * 300)  # delivered, not inserted, the table emptied
    # size update to 0 and back, twice in front of the first field
    fields, res = one(h, size_update(0) + size_update(256) + literal(b"d", b"4"), sid=3)
    assert res[3:6] == (1, 1, 34) and h.model.table.entries == [(b"d", b"4")]
    fields, res = one(h, size_update(40, extra=1) + indexed(62) + literal(b"e", b"55555"), sid=5)
    assert res[3:6] == (1, 1, 38) and h.model.table.max_size == 40
    h.close()


def test_a_name_reference_to_the_entry_its_insertion_evicts(gpu):
    h = HH(gpu, setting=100)
    one(h, size_update(100) + literal(b"name-of-fifteen", b"v" * 20))  # 67 bytes
    fields, res = one(h, literal(62, b"w" * 21), sid=3)  # RFC 7541 4.4: the name is read before the entry goes
    assert fields == [(b"name-of-fifteen", b"w" * 21, 1)] and res[3:6] == (1, 1, 68)
    # the entry just evicted is no longer there
    failing(h, indexed(63), ERR_INDEX, sid=5)
    h.close()


def test_the_setting_lowered_then_a_size_update_above_it(gpu):
    h = HH(gpu)
    one(h, literal(b"a", b"1") + literal(b"b", b"2"))
    h.set_max_table_size(40)  # (at once: one entry goes)
    assert h.model.table.entries == [(b"b", b"2")] and h.model.stats["evicted"] == 1
    assert one(h, size_update(40) + indexed(62), sid=3)[0] == [(b"b", b"2", 0)]
    h.set_max_table_size(8192)
    assert one(h, size_update(8192) + indexed(62), sid=5)[1][6] == 0
    h.set_max_table_size(100)
    failing(h, size_update(101) + indexed(62), ERR_SIZE_UPDATE, sid=7)
    h.close()


@pytest.mark.parametrize("case", ["index 0", "beyond the table", "ten continuation bytes", "2^32", "a string past the end",
                                  "an integer past the end", "a size update behind a field", "a size update above the setting"])
def test_malformed_blocks(gpu, case):
    h = HH(gpu)
    block, err = {
        "index 0": (b"\x82\x80", ERR_INDEX),
        "beyond the table": (literal(b"a", b"1") + indexed(63), ERR_INDEX),
        "ten continuation bytes": (b"\x82\xff" + b"\xff" * 10 + b"\x00", ERR_INTEGER),
        "2^32": (b"\xff" + b"\x81\xff\xff\xff\x0f", ERR_INTEGER),
        "a string past the end": (b"\x82\x00\x01a\x05abcd", ERR_TRUNCATED),
        "an integer past the end": (b"\x82\xff\x80", ERR_TRUNCATED),
        "a size update behind a field": (b"\x82" + size_update(100), ERR_SIZE_UPDATE),
        "a size update above the setting": (size_update(4097) + b"\x82", ERR_SIZE_UPDATE),
    }[case]
    failing(h, block, err)
    h.close()


# ---- block size and errors -------------------------------------------------------------------------------------------------
def test_a_block_of_exactly_max_block_bytes_and_one_more(gpu):
    h = HH(gpu, max_block=64)
    exact = literal(b"k", b"v" * 60, mode=2)  # 1 + 2 + 1 + 60
    assert len(exact) == 64
    wire = headers_frames(1, exact, cont=(30,))
    assert h.feed([wire[:50]])[1][6] == OPEN  # (the carry holds what it may)
    assert h.feed([wire[50:]])[0] == [(1, 0, [(b"k", b"v" * 60, 2)])]
    blocks, res = h.feed([headers_frames(3, b"\x82") + headers_frames(5, literal(b"k", b"v" * 61, mode=2)) + headers_frames(7, b"\x82")])
    assert len(blocks) == 1 and res[6] == word(FAILED, ERR_BLOCK_TOO_LARGE, 5)
    h.close()
    # ... and a block that grows past it while it is open
    h = HH(gpu, max_block=64)
    wire = headers_frames(1, literal(b"k", b"v" * 100, mode=2))
    assert h.feed([wire[:9 + 65]])[1][6] == word(FAILED, ERR_BLOCK_TOO_LARGE, 1)
    h.close()


def test_an_error_in_the_third_block_of_five(gpu):
    h = HH(gpu)
    wire = b"".join(headers_frames(2 * k + 1, literal(b"n%d" % k, b"v") if k != 2 else literal(b"n2", b"v") + b"\x80") for k in range(5))
    blocks, res = h.feed([wire])
    assert [b[0] for b in blocks] == [1, 3] and res == (2, 2, 6, 2, 0, 70, word(FAILED, ERR_INDEX, 5), 0)
    assert h.model.table.entries == [(b"n1", b"v"), (b"n0", b"v")]  # (what the failing block inserted is not there)
    for _ in range(2):
        assert h.feed([headers_frames(11, b"\x82")])[1] == (0, 0, 0, 0, 0, 70, word(FAILED, ERR_INDEX, 5), 0)
    assert h.model.stats["calls"] == 3
    h.close()


# ---- caps and lifetime -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("short", [0, 1, 2], ids=["blocks", "fields", "strings"])
def test_cap_overflows_and_their_repeat(gpu, short):
    h = HH(gpu)
    cut = headers_frames(9, literal(b"tail", b"t" * 20))
    h.feed([headers_frames(1, literal(b"a", b"1")) + cut[:15]])  # a cut block in the carry
    wire = cut[15:] + headers_frames(3, indexed(62) + indexed(63)) + headers_frames(5, literal(b"c", b"3")) + cut[:12]
    h.deframe([wire])
    caps = [3, 4, 52]
    caps[short] -= 1
    before = (list(h.model.table.entries), dict(h.model.stats))
    res = h.decode(tuple(caps))[1]
    assert res[:3] == (3, 4, 52) and res[7] == 1 and (list(h.model.table.entries), h.model.stats) == before
    blocks, res = h.decode((3, 4, 52))  # (the same call, with room: exact caps)
    assert res == (3, 4, 52, 2, 0, h.model.table.size, OPEN, 0) and [b[0] for b in blocks] == [9, 3, 5]
    assert h.feed([cut[12:]])[0][0][2] == [(b"tail", b"t" * 20, 1)]
    h.close()


def test_lost_and_skipped_calls_and_a_deframer_error(gpu):
    h = HH(gpu)
    h.feed([headers_frames(1, literal(b"a", b"1"))])
    with pytest.raises(gpu.GrdmaError, match=ERR5):
        h.deframe([headers_frames(3, b"\x82") * 8], ev_cap=4, checked=False)  # the event list overflows
    h.lost = True
    assert h.decode()[1] == (0, 0, 0, 0, 0, 34, LOST, 2)
    h.deframe([headers_frames(5, b"\x82")], checked=False)  # (the parser lost its place in the overflowing call)
    assert h.decode()[1] == (0, 0, 0, 0, 0, 34, LOST, 0) and h.model.stats["calls"] == 3
    h.close()
    h = HH(gpu)
    h.deframe([headers_frames(1, literal(b"a", b"1"))])  # never taken in
    h.deframe([headers_frames(3, b"\x82")])
    h.skipped = True
    assert h.decode()[1][6:] == (LOST, 0)
    h.close()
    h = HH(gpu)
    h.deframe([headers_frames(1, b"\x82") + frame(9, 4, 1, b"\x82")])  # a CONTINUATION out of place: a connection error
    assert h.last[0] != 0 and h.decode()[1] == (0, 0, 0, 0, 0, 0, word(FAILED, ERR_DEFRAMER), 0)
    h.close()


@pytest.mark.parametrize("first", ["decoder", "others"])
def test_control_writer_and_send_windows_on_the_same_deframing(gpu, first):
    from grpc_rdma_amd import h2dev
    from tests.h2_control_lib import Target
    from tests.h2_control_model import ControlModel
    from tests.h2_send_model import SendModel, live_of
    h = HH(gpu, streams=(1, 3))
    ctl, cm = h2dev.ControlReplies(h.parser), ControlModel()
    sw, sm = h2dev.SendWindows(h.parser), SendModel()
    hd = headers_frames(1, literal(b"k", b"v" * 30) + indexed(62))
    calls = ([settings(1) + ping(5) + hd[:20]], [hd[20:] + data(3, b"y" * 50) + bad_flags(3) + ping(6) + headers_frames(3, indexed(62))])
    for slices in calls:
        h.deframe(slices)
        err_o, ev_o = h.last
        t = Target(gpu, 8)

        def others():
            lens, wire, res = cm.reply(ev_o, slices, err_o, 8, 256)
            sl, got = ctl.reply(t.slices.ptr, 8, t.hdr.ptr, 256)
            same(got, res, "writer: result")
            t.check(gpu, sl, lens, wire, "writer")
            same(sw.intake(), sm.intake(ev_o, slices, err_o, live_of(h.pp.orc)), "intake: result")

        for step in ((h.decode, others) if first == "decoder" else (others, h.decode)):
            step()
    assert h.model.stats["blocks"] == 2 and h.model.stats["fields"] == 3 and cm.stats["ping_acks"] == 2
    ctl.close()
    sw.close()
    h.close()


def test_refusals_and_lifetime(gpu):
    from grpc_rdma_amd import h2dev
    h = HH(gpu)
    t = Targets(gpu, 4, 8, 64)
    with pytest.raises(gpu.GrdmaError, match="already"):
        h2dev.HeaderDecoder(h.parser)
    p2 = h2dev.Parser(False, 16384)
    for args, why in (((65537, 4096), "max_table_size"), ((4096, 63), "max_block_bytes"), ((4096, (1 << 20) + 1), "max_block_bytes")):
        with pytest.raises(gpu.GrdmaError, match=why):
            h2dev.HeaderDecoder(p2, *args)
    h2dev.HeaderDecoder(p2, 65536, 1 << 20).close()
    h2dev.HeaderDecoder(p2, 0, 64).close()
    p2.close()
    with pytest.raises(gpu.GrdmaError, match="deframed nothing"):
        h.dec.decode(*t.args())
    with pytest.raises(gpu.GrdmaError):
        h.dec.set_max_table_size(65537)
    h.deframe([headers_frames(1, b"\x82\x86")])
    good = t.args()
    for k in range(6):
        bad = list(good)
        bad[k] = 0
        with pytest.raises(gpu.GrdmaError, match="null, zero or misaligned"):
            h.dec.decode(*bad)
    for k in (0, 2, 4):
        bad = list(good)
        bad[k] += 8
        with pytest.raises(gpu.GrdmaError, match="null, zero or misaligned"):
            h.dec.decode(*bad)
    assert t.read() == tuple(bytes([0xA5]) * len(x) for x in t.read())  # (untouched)
    n, res = h.dec.decode(*good)  # (nothing changed: the call is still to be taken)
    assert (n, res) == (1, (1, 2, 21, 0, 0, 0, 0, 0)) and h.dec.stats()["calls"] == 1
    with pytest.raises(gpu.GrdmaError, match="taken in already"):
        h.dec.decode(*good)
    # a parser that is gone: every call is refused, destroy still works
    h.parser.close()
    with pytest.raises(gpu.GrdmaError, match="parser is gone"):
        h.dec.decode(*good)
    assert h.dec.stats()["fields"] == 2 and h.dec.table()[0] == []
    h.dec.close()
    h.dec.close()
