"""The header decoder (k_h2_hpack_gather / _copy / _split / _walk / _emit / _commit / _resize, csrc/grdma_h2_hpack.h and
csrc/grdma_h2_hpack_stage.inc) swept over header blocks built from the constants it branches on: 256 threads, 512 staged
records, a ring of 2048 descriptors, a byte ring of 65536, the prefix widths 4 / 5 / 6 / 7, 62 static entries, 32 bytes of
entry overhead (numbers: profiles/h2_hpack_sweep.md).

A case is a deterministic script of steps on one HH harness (tests/h2_hpack_lib.py): ("feed", slices[, ev_cap[, caps]]),
("resize", n), ("decode", caps) -- the repeat of a call that overflowed a cap.  The reference is
tests/h2_hpack_model.HpackModel; HH.feed / HH.decode compare the three targets whole with their sentinels, the result
block, the dynamic table and the counters exactly.  Nothing here has a tolerance.

Every case names the edge it is there for, and a witness -- computed from the model alone (simulate) -- shows that the
case reaches it; check_cases() runs them all.  pytest rewrites no `assert` in a helper module: checks go through `same`."""
import copy
import functools

from oracle import pyorc
from tests.h2_control_lib import ping
from tests.h2_device_lib import oracle_feed, same
from tests.h2_helpers import frame
from tests.h2_hpack_lib import enc_int, enc_str, headers_frames, huff, indexed, literal, size_update
from tests.h2_hpack_model import (BYTES, CHUNK, ERR_HUFFMAN, ERR_INDEX, ERR_INTEGER, ERR_PADDING, ERR_SIZE_UPDATE, ERR_TRUNCATED, FAILED,
                                  HUFFMAN, OPEN, RING, THREADS, HpackModel, RingLayout, block_facts, gather_steps, header_items,
                                  split, walk_steps)

FAMILIES = ("01", "02", "03", "04", "05", "06", "07", "08", "09", "10")
PINNED = ("01", "02", "04", "05", "06", "07", "09")  # the families whose block sequences go through nghttp2 as well
CAPS = (1024, 8192, 1 << 17)
SIZES = (511, 512, 513, 1023, 1024, 1025, 1537)
RUNS = (255, 256, 257, 512, 513)
BIG = (1 << 24) - 1, 1 << 24, (1 << 24) + 2, (1 << 25) + 62, (1 << 28) + 2  # what would alias w0's bits above the index
# cases that were the only ones to catch a change of the mutation table (profiles/h2_hpack_sweep.md)
CAUGHT_ALONE = ["01_two_size_updates_600_fields", "02_big_block_between_small", "03_payload_events_cross_a_step_open",
                "05_three_entries_past_half"]
# Where nghttp2 refuses a block sequence the model takes, because of a limit of its own: case id -> the reason.  Nothing of
# families 4, 5 and 7 may stand here, and no case on which nghttp2 takes a block the model refuses.
NGHTTP2_DIFFERS = {}

CASES = []


def case(fam, name, edge, key, steps, wit, setting=4096, max_block=65536, caps=CAPS):
    """key: the edge's kind within the family (emu_subset takes the smallest case of each); wit(sim) -> truth, sim =
    simulate(c); a cap may be ("need", (d blocks, d fields, d string bytes)): what the call needs plus that"""
    CASES.append(dict(id="%s_%s" % (fam, name), fam=fam, edge=edge, key=key, steps=steps, wit=wit, setting=setting, max_block=max_block,
                      caps=caps))


# ---- builders ---------------------------------------------------------------------------------------------------------
def cuts(block):
    return tuple(range(16384, len(block), 16384))


def wire_of(blocks, sid=1):
    """every block in frames of its own (CONTINUATIONs where it is longer than a frame), streams sid, sid + 2, ..."""
    return b"".join(headers_frames(sid + 2 * k, b, cont=cuts(b)) for k, b in enumerate(blocks))


def feed(blocks, sid=1):
    w = wire_of(blocks, sid)
    return ("feed", [w], max(4096, 4 * len(blocks) + 64))


def static_run(n, start=0):
    return b"".join(indexed(2 + (start + j) % 60) for j in range(n))


def pat(n, seed):
    return bytes((seed * 29 + 7 * i + (i >> 8)) % 251 for i in range(n))


def chunks(n):
    return [CHUNK] * (n // CHUNK) + ([n % CHUNK] if n % CHUNK else [])


def word(flags, err=0, stream=0):
    return flags | err << 8 | stream << 32


def failed(s, err, stream):
    return s["res"][6] == word(FAILED, err, stream) and s["res"][7] == 0


def bits(data, tail):
    """the Huffman codes of data and behind them the bit string tail ('E': the 30 ones of EOS) -> bytes; must end on a byte"""
    acc = "".join(format(HUFFMAN[b][0], "0%db" % HUFFMAN[b][1]) for b in data) + tail.replace("E", "1" * 30)
    if len(acc) % 8:
        raise ValueError("%d bits do not end on a byte" % len(acc))
    return int(acc, 2).to_bytes(len(acc) // 8, "big") if acc else b""


def raw_huff(body):
    return enc_int(len(body), 7, 0x80) + body


# ---- the model alone --------------------------------------------------------------------------------------------------
def _caps_of(spec, model, ev, slices):
    if spec[0] != "need":
        return spec
    need = copy.deepcopy(model).decode(ev, slices, 0, (1 << 40, 1 << 40, 1 << 40))[3]
    return tuple(need[i] + spec[1][i] for i in range(3))


@functools.lru_cache(maxsize=None)
def _simulate(cid):
    c = by_id(cid)
    orc = pyorc.H2Parser(expect_client_prefix=False)
    model, ring, setting = HpackModel(c["setting"], c["max_block"]), RingLayout(), c["setting"]
    out, last = [], None
    for st in c["steps"]:
        if st[0] == "resize":
            model.set_max_table_size(st[1])
            ring.commit(model.table, 0)
            setting = st[1]
            out.append(dict(kind="resize", entries=len(model.table.entries), size=model.table.size, evicted=model.table.evicted))
            continue
        if st[0] == "feed":
            err, ev = oracle_feed(orc, st[1])
            same(err, 0, "%s: the fed bytes' h2 error" % cid)
            same(len(ev) <= ((st[2] if len(st) > 2 else None) or 8 * len(st[1]) + 4096), True, "%s: the events fit the event cap" % cid)
            last, spec = (ev, st[1]), (st[3] if len(st) > 3 else None) or c["caps"]
        else:
            spec = st[1]
        ev, slices = last
        caps = _caps_of(spec, model, ev, slices)
        carried, ins0, head0 = model.block is not None, model.table.inserted, ring.head
        blocks, fields, strings, res, rc = model.decode(ev, slices, 0, caps)
        if res[7] == 0:
            ring.commit(model.table, res[3])
        facts = [block_facts(b, setting) for b in model.closed]
        good = next((i for i, f in enumerate(facts) if f is None), len(facts))
        out.append(dict(kind=st[0], caps=caps, res=res, rc=rc, blocks=blocks, nfields=len(fields), closed=list(model.closed), facts=facts,
                        nrec=[f[0] for f in facts[:good]], steps=walk_steps([f[0] for f in facts[:good]]), nev=len(ev),
                        gather=gather_steps(len(ev)), hdr=header_items(ev, carried), carried=carried, ins0=ins0,
                        ins1=model.table.inserted, head0=head0, head1=ring.head, where=list(ring.where), straddles=ring.straddles(),
                        entries=len(model.table.entries), size=model.table.size, table=list(model.table.entries[:4]),
                        records=sum(f[0] for f in facts if f)))
    return out


def simulate(c):
    """-> per step what the model alone says: the call's events and header items, the blocks it completes and their
    records, the walk's and the gather's steps, insertions and the byte ring's head in front and behind, the result"""
    return _simulate(c["id"])


# ---- family 1: records per block around the chunk ----------------------------------------------------------------------
def fam01():
    for n in SIZES:
        case("01", "indexed_%d" % n, "one block of %d indexed fields: one parallel run per chunk" % n, "indexed", [feed([static_run(n)])],
             lambda sim, n=n: sim[0]["nrec"] == [n] and [s[3] for s in sim[0]["steps"]] == chunks(n) and sim[0]["res"][:2] == (1, n)
             and (n <= CHUNK) == (sim[0]["steps"][0][1] == 1))
        block = b"".join(literal(b"k", b"%d" % j) for j in range(n))
        case("01", "inserting_%d" % n, "one block of %d inserting literals: every record a one-thread step" % n, "inserting", [feed([block])],
             lambda sim, n=n: sim[0]["nrec"] == [n] and [s[3] for s in sim[0]["steps"]] == chunks(n) and sim[0]["res"][3] == n
             and sim[0]["res"][4] > 0)
    for r in (510, 511, 512, 513):
        block = static_run(r) + literal(b"seam", b"at%d" % r) + b"".join(indexed(62) if j % 2 else literal(62, b"v%d" % j, mode=2)
                                                                          for j in range(1025 - r - 1))
        case("01", "insertion_at_%d" % r, "1025 records, the one insertion is record %d: the fields behind it reference it across the "
             "seam at 512" % r, "seam", [feed([block])],
             lambda sim, r=r: sim[0]["nrec"] == [1025] and sim[0]["res"][3] == 1 and [f[0] for f in split(sim[0]["closed"][0], 4096)].index(1) == r
             and all(f[1] == 62 for f in split(sim[0]["closed"][0], 4096)[r + 1:]) and sim[0]["res"][:2] == (1, 1025))
    block = size_update(0) + size_update(4096) + static_run(600)
    case("01", "two_size_updates_600_fields", "two size updates, then 600 fields, and a block behind: records and fields differ across the seam", "size",
         [feed([literal(b"gone", b"x")]), feed([block, indexed(2)], 3)],
         lambda sim: sim[1]["facts"] == [(602, 600, 2), (1, 1, 0)] and [s[3] for s in sim[1]["steps"]] == [512, 90, 1] and sim[1]["res"][4] == 1
         and sim[1]["blocks"][1][1] == 600)
    block = literal(b"chain", b"0") + b"".join(literal(62, b"%d" % j) for j in range(1, 520))
    case("01", "name_chain_across_the_seam", "520 insertions, each naming the entry the record in front inserted", "chain", [feed([block])],
         lambda sim: sim[0]["nrec"] == [520] and sim[0]["res"][3] == 520 and sim[0]["table"][0] == (b"chain", b"519")
         and [s[3] for s in sim[0]["steps"]] == [512, 8])


# ---- family 2: blocks per walk step ------------------------------------------------------------------------------------
def fam02():
    for r in (0, 1, 2):
        for n in RUNS:
            case("02", "%d_blocks_of_%d" % (n, r), "%d blocks of %d records: a step takes %d blocks at most" % (n, r, THREADS),
                 "run%d" % r, [feed([static_run(r, k) for k in range(n)])],
                 lambda sim, r=r, n=n: [s[1] for s in sim[0]["steps"]] == [THREADS] * (n // THREADS) + ([n % THREADS] if n % THREADS else [])
                 and sim[0]["nrec"] == [r] * n and sim[0]["res"][:2] == (n, r * n))
    for last, want in ((112, [3, 1]), (113, [2, 2])):
        case("02", "sum_lands_on_%d" % (400 + last), "blocks of 200, 200, %d, 5 records: the running sum lands on %d" % (last, 400 + last),
             "sum", [feed([static_run(200), static_run(200, 7), static_run(last, 3), static_run(5)])],
             lambda sim, want=want, last=last: [s[1] for s in sim[0]["steps"]] == want and sim[0]["nrec"] == [200, 200, last, 5])
    small = lambda k: literal(b"s%d" % k, b"v") + indexed(62) + indexed(2)  # noqa: E731
    big = b"".join(indexed(62 + j % 2) if j % 3 else literal(63, b"b%d" % j, mode=3) for j in range(600))
    case("02", "big_block_between_small", "blocks of 3, 3, 600, 3, 3 records: whole blocks, then chunks, then whole blocks again", "big",
         [feed([small(0), small(1), big, small(2), small(3)])],
         lambda sim: sim[0]["steps"] == [(0, 2, 0, 6), (2, 0, 0, 512), (2, 0, 512, 88), (3, 2, 0, 6)] and sim[0]["res"][:2] == (5, 612))
    x = lambda k: indexed(2 + k) + indexed(3)  # noqa: E731
    for name, blocks in (("first", [b"", x(0), x(1)]), ("last", [x(0), x(1), b""]), ("consecutive", [x(0), b"", b"", x(1)])):
        case("02", "empty_block_%s" % name, "a HEADERS frame with an empty fragment: " + name, "empty", [feed(blocks)],
             lambda sim, blocks=blocks: sim[0]["nrec"] == [len(b) for b in blocks] and sim[0]["res"][0] == len(blocks))
    case("02", "empty_block_open_then_closed_empty", "an empty HEADERS frame leaves its block open; an empty CONTINUATION closes it in the next call",
         "empty", [("feed", [wire_of([x(0)]) + frame(1, 0, 3, b"")]), ("feed", [frame(9, 4, 3, b"") + wire_of([x(1)], 5)])],
         lambda sim: sim[0]["res"][6] == OPEN and sim[0]["nrec"] == [2] and sim[1]["carried"] and sim[1]["nrec"] == [0, 2]
         and sim[1]["blocks"][0][:3] == (3, 0, 0) and sim[1]["res"][6] == 0)


# ---- family 3: items per gather step ------------------------------------------------------------------------------------
def front(nev, sid):
    """header blocks of their own that make nev events, as slices (an odd count: one payload is cut in two) -> (slices, next stream)"""
    out, n = [], nev // 2
    if nev % 2:
        w = headers_frames(sid, b"\x82\x84")
        out, sid, n = [w[:10], w[10:]], sid + 2, n - 1
    rest = b"".join(headers_frames(sid + 2 * k, b"\x82") for k in range(n))
    if out:
        return [out[0], out[1] + rest], sid + 2 * n
    return [rest], sid + 2 * n


def fam03():
    for t in (THREADS - 1, THREADS, THREADS + 1):
        sl, sid = front(t - 1, 1)
        sl[-1] += headers_frames(sid, literal(b"at", b"%d" % t) + indexed(62))
        case("03", "headers_at_item_%d" % t, "a HEADERS frame is item %d of a call without carry" % t, "headers", [("feed", sl)],
             lambda sim, t=t: sim[0]["hdr"][-1] == t and not sim[0]["carried"] and sim[0]["nev"] == t + 1 and sim[0]["res"][3] == 1)
        sl, sid = front(t - 3, 1)
        sl[-1] += headers_frames(sid, literal(b"at", b"%d" % t) + indexed(62) + indexed(4), cont=(6,))
        case("03", "continuation_at_item_%d" % t, "a block's CONTINUATION is item %d, its HEADERS frame item %d" % (t, t - 2), "continuation",
             [("feed", sl)], lambda sim, t=t: sim[0]["hdr"][-2:] == [t - 2, t] and sim[0]["res"][1] == (t - 3) // 2 + (t - 3) % 2 + 3)
        # a carried block first: item 0 is a header frame, and the frame at item t is behind t - 1 events all the same
        sl, sid = front(t - 3, 3)
        sl[0] = frame(9, 4, 1, indexed(62)) + sl[0]
        sl[-1] += headers_frames(sid, indexed(62) + indexed(5))
        case("03", "carry_then_headers_at_item_%d" % t, "a carried block is item 0; a HEADERS frame is item %d" % t, "carry",
             [("feed", [frame(1, 0, 1, literal(b"open", b"block"))]), ("feed", sl)],
             lambda sim, t=t: sim[1]["carried"] and sim[1]["hdr"][0] == 0 and sim[1]["hdr"][-1] == t and sim[1]["res"][6] == 0
             and sim[0]["res"][6] == OPEN)
        # the carried block goes on through CONTINUATION frames of one byte and closes at item t
        n = (t - 1) // 2 - (t - 1) % 2
        frames_ = [frame(9, 0, 1, indexed(2 + k % 60)) for k in range(n)]
        if (t - 1) % 2:
            w = frame(9, 0, 1, indexed(7) + indexed(8))
            sl = [w[:10], w[10:] + b"".join(frames_)]
        else:
            sl = [b"".join(frames_)]
        sl[-1] += frame(9, 4, 1, indexed(62))
        case("03", "carried_block_closes_at_item_%d" % t, "a carried block of %d CONTINUATION frames closes at item %d" % (n + 1 + (t - 1) % 2, t), "chain",
             [("feed", [frame(1, 0, 1, literal(b"open", b"block"))]), ("feed", sl)],
             lambda sim, t=t, n=n: sim[1]["hdr"][-1] == t and len(sim[1]["closed"]) == 1 and sim[1]["res"][:2] == (1, n + 2 + (t - 1) % 2 * 2))
    block = literal(b"one-byte", b"slices") + static_run(20) + indexed(62)
    w = headers_frames(501, block)
    sl, _ = front(THREADS - 8, 1)
    whole = sl + [w[i:i + 1] for i in range(len(w))]
    case("03", "payload_events_cross_a_step_complete", "a frame in one-byte slices: its PAYLOAD events cross item %d, it completes" % THREADS,
         "bytes", [("feed", whole)],
         lambda sim: sim[0]["hdr"][-1] == THREADS - 7 and sim[0]["nev"] > THREADS + 20 and sim[0]["res"][6] == 0 and len(sim[0]["gather"]) == 2)
    case("03", "payload_events_cross_a_step_open", "the same, and the call ends inside the payload: the block is open", "bytes",
         [("feed", whole[:-12]), ("feed", whole[-12:])],
         lambda sim: sim[0]["hdr"][-1] == THREADS - 7 and sim[0]["nev"] > THREADS + 8 and sim[0]["res"][6] == OPEN and sim[1]["carried"]
         and sim[1]["res"][:2] == (1, 22))
    sl, sid = front(100, 1)
    sl[-1] += headers_frames(sid, literal(b"last", b"header frame")) + b"".join(ping(k) for k in range(220))
    case("03", "last_header_frame_in_an_earlier_step", "the last header frame closes its block in step 0, the call's events go on through step 1",
         "last", [("feed", sl)],
         lambda sim: sim[0]["hdr"][-1] == 101 and len(sim[0]["gather"]) >= 2 and sim[0]["nev"] > 2 * THREADS and sim[0]["res"][6] == 0)
    case("03", "carry_and_300_blocks", "a carried open block and 300 further blocks", "carry",
         [("feed", [frame(1, 0, 1, literal(b"open", b"block"))]),
          ("feed", [frame(9, 4, 1, indexed(62)) + wire_of([indexed(62) + indexed(2 + k % 60) for k in range(300)], 3)])],
         lambda sim: sim[1]["carried"] and sim[1]["res"][:2] == (301, 602) and len(sim[1]["gather"]) == 3)


# ---- family 4: the descriptor ring ---------------------------------------------------------------------------------------
def fam04():
    ins = lambda a, b: b"".join(literal(b"", b"%d" % j) for j in range(a, b))  # noqa: E731
    reads = lambda n: b"".join(indexed(62 + j) for j in range(n))  # noqa: E731
    for total in (RING, 2 * RING):
        n = total + 52
        case("04", "%d_insertions_in_one_call" % n, "%d insertions in one call, then every live entry by index: live entries on both "
             "sides of slot %d" % (n, total % RING), "wrap%d" % total, [feed([ins(0, n), reads(100)])],
             lambda sim, n=n, total=total: sim[0]["ins1"] == n and sim[0]["entries"] >= 100 and (n - 100) < total < n - 1)
        third = n // 3 + 1
        case("04", "%d_insertions_across_calls" % n, "the same across three calls", "wrap%d" % total,
             [feed([ins(k * third, min(n, (k + 1) * third)), reads(100)]) for k in range(3)],
             lambda sim, n=n, total=total: sim[2]["ins1"] == n and sim[2]["ins0"] < total < n - 1 and sim[2]["entries"] >= 100 and n - 100 < total)
    full = size_update(65536) + literal(b"", b"") * RING
    fill = feed([full])
    is_full = lambda s: s["entries"] == RING and s["size"] == 65536  # noqa: E731
    case("04", "full_table_the_oldest", "2048 live entries of 32 bytes; index 62 + 2047 is the oldest", "full",
         [fill, feed([indexed(62) + indexed(62 + RING - 1)], 3)], lambda sim: is_full(sim[0]) and sim[1]["res"][:2] == (1, 2) and is_full(sim[1]),
         setting=65536)
    case("04", "full_table_one_beyond", "2048 live entries; index 62 + 2048 is none", "full",
         [fill, feed([indexed(62 + RING - 1) + indexed(62 + RING)], 3)],
         lambda sim: is_full(sim[0]) and failed(sim[1], ERR_INDEX, 3) and is_full(sim[1]), setting=65536)
    case("04", "full_table_insert_2049th", "the 2049th insertion evicts exactly one entry and takes the slot of the oldest", "full",
         [fill, feed([literal(62 + RING - 1, b"") + indexed(62) + indexed(62 + RING - 1), literal(b"", b"y") + indexed(62 + RING - 2)], 3)],
         lambda sim: is_full(sim[0]) and sim[1]["res"][3:5] == (2, 3) and sim[1]["ins1"] == RING + 2 and sim[1]["entries"] == RING - 1,
         setting=65536)
    for n in (0, 64):
        case("04", "full_table_resize_to_%d" % n, "our setting lowered to %d on the full table" % n, "resize",
             [fill, ("resize", n), feed([size_update(n) + (indexed(63) if n else indexed(2)) + literal(b"", b"after")], 3)],
             lambda sim, n=n: is_full(sim[0]) and sim[1]["entries"] == n // 32 and sim[1]["evicted"] == RING - n // 32 and sim[2]["res"][0] == 1,
             setting=65536)
    case("04", "resize_between_wraps", "the setting lowered and raised while the ring wraps: evictions read slots on both sides of 2047", "resize",
         [feed([ins(0, 2040)]), ("resize", 300), feed([size_update(300) + ins(2040, 2060) + reads(6)], 3), ("resize", 4096),
          feed([size_update(4096) + ins(2060, 2100) + reads(40)], 5)],
         lambda sim: sim[0]["ins1"] == 2040 and 0 < sim[1]["entries"] < 10 and sim[2]["ins1"] == 2060 and sim[4]["ins1"] == 2100)


# ---- family 5: the byte ring ---------------------------------------------------------------------------------------------
def fam05():
    # sixteen calls insert one entry of 2000 + 2000 string bytes each (the table holds one): the head stands at 64000
    lead = [feed([literal(pat(2000, 2 * k), pat(2000, 2 * k + 1))], 1 + 2 * k) for k in range(16)]
    for what, nl, vl in (("name", 2000, 2000), ("value", 1000, 3000), ("between", 1536, 2000)):
        case("05", "%s_straddles" % what, "at setting 4096 the seventeenth entry stands at offset 64000 of the byte ring: %s lies across "
             "65536; read back by index in the next call" % {"name": "its name", "value": "its value", "between": "the seam of name and value"}[what],
             "straddle", lead + [feed([literal(pat(nl, 40), pat(vl, 41))], 41), feed([indexed(62) + literal(62, b"short", mode=2)], 43),
                                 feed([literal(62, b"x" * 10) + indexed(62) + indexed(63)], 45)],
             lambda sim, what=what: sim[16]["head0"] == 64000 and sim[16]["straddles"] == [(62, what)] and sim[17]["straddles"] == [(62, what)]
             and sim[17]["res"][:2] == (1, 2) and sim[18]["head1"] < 4096 and sim[18]["entries"] == 1)
    nl, vl = 30000, 65536 - 32 - 30000
    big = size_update(65536) + literal(pat(nl, 5), pat(vl, 6))
    case("05", "one_entry_fills_the_byte_ring", "setting 65536: one entry of 65536 - 32 string bytes, then an insertion that names it and "
         "evicts it: the new name lies across 65536", "fill",
         [feed([big]), feed([indexed(62)], 3), feed([literal(62, b"v") + indexed(62)], 5)],
         lambda sim: sim[0]["size"] == 65536 and sim[0]["head1"] == 65504 and sim[2]["res"][3:5] == (1, 1) and sim[2]["straddles"] == [(62, "name")]
         and sim[2]["head1"] == (65504 + nl + 1) % BYTES, setting=65536, max_block=1 << 17, caps=(16, 64, 1 << 18))
    case("05", "three_entries_past_half", "setting 65536: entries of 20000, 20000 and 10000 string bytes from three calls are alive together, "
         "the third stands behind offset 32768; all read back by index", "half",
         [feed([size_update(65536) + literal(pat(8000, 1), pat(12000, 2))]), feed([literal(pat(12000, 3), pat(8000, 4))], 3),
          feed([literal(pat(5000, 5), pat(5000, 6))], 5), feed([indexed(64) + indexed(63) + indexed(62)], 7)],
         lambda sim: sim[2]["where"] == [(40000, 5000, 5000), (20000, 12000, 8000), (0, 8000, 12000)] and sim[3]["res"][:3] == (1, 3, 50000)
         and sim[3]["entries"] == 3, setting=65536, max_block=1 << 17, caps=(16, 64, 1 << 18))
    case("05", "one_entry_fills_then_small", "the same entry, then a small insertion in a later call: its strings stand behind the big one's",
         "fill", [feed([big]), feed([literal(b"small", b"one") + indexed(62)], 3), feed([indexed(62)], 5)],
         lambda sim: sim[0]["head1"] == 65504 and sim[1]["res"][3:5] == (1, 1) and sim[1]["where"] == [(65504, 5, 3)],
         setting=65536, max_block=1 << 17, caps=(16, 64, 1 << 18))


# ---- family 6: integers ---------------------------------------------------------------------------------------------------
def fill_table(n):
    """a block that leaves n entries (x<j>, y), the newest x<n-1>"""
    return b"".join(literal(b"x%d" % j, b"y") for j in range(n))


def fam06():
    ok = lambda nf: (lambda sim: sim[-1]["res"][0] == len(sim[-1]["closed"]) and sim[-1]["res"][1] == nf and sim[-1]["res"][6] == 0)  # noqa: E731
    for v in (14, 15, 16):
        for mode in (2, 3):
            case("06", "w4_static_name_%d_mode%d" % (v, mode), "4-bit prefix: the static name index %d" % v, "w4",
                 [feed([literal(v, b"val", mode=mode)])], ok(1))
    for v in (30, 31, 32):
        case("06", "w5_size_update_%d" % v, "5-bit prefix: a size update to %d" % v, "w5", [feed([literal(b"gone", b"x")]),
                                                                                               feed([size_update(v) + indexed(2)], 3)],
             lambda sim, v=v: sim[1]["res"][4] == 1 and sim[1]["facts"] == [(2, 1, 1)])
    for v in (62, 63, 64):
        case("06", "w6_dynamic_name_%d" % v, "6-bit prefix: the dynamic name index %d" % v, "w6", [feed([fill_table(3), literal(v, b"val")])],
             lambda sim, v=v: sim[0]["res"][:2] == (2, 4) and sim[0]["table"][0] == (b"x%d" % (2 - (v - 62)), b"val"))
    for v in (126, 127, 128):
        case("06", "w7_dynamic_index_%d" % v, "7-bit prefix: the dynamic index %d" % v, "w7", [feed([fill_table(70), indexed(v)])],
             lambda sim, v=v: sim[0]["res"][:2] == (2, 71) and sim[0]["entries"] == 70)
        for which in ("name", "value"):
            for h in (False, True):
                k = next(k for k in range(2 * v) if len(huff(b"n" * k)) == v) if h else v  # (the prefix counts the bytes on the wire)
                body = enc_str(b"n" * k, h)
                block = (b"\x10" + body + enc_str(b"v")) if which == "name" else (b"\x10" + enc_str(b"n") + body)
                case("06", "w7_%s_length_%d%s" % (which, v, "_huffman" if h else ""), "7-bit prefix: a %s of %d bytes on the wire" % (which, v),
                     "w7len", [feed([block])], ok(1))
    # non-minimal forms: five continuation bytes are taken, six are not
    table = fill_table(70)
    five = {"w4": literal(16, b"v", mode=2, extra=4), "w5": size_update(100, extra=4) + indexed(2), "w6": literal(63, b"v", extra=4),
            "w7": indexed(128, extra=4), "w7len": b"\x10" + enc_int(127, 7, 0, 4) + b"n" * 127 + enc_str(b"v")}
    six = {"w4": literal(16, b"v", mode=2, extra=5), "w5": size_update(100, extra=5) + indexed(2), "w6": literal(63, b"v", extra=5),
           "w7": indexed(128, extra=5), "w7len": b"\x10" + enc_int(127, 7, 0, 5) + b"n" * 127 + enc_str(b"v")}
    for w in five:
        case("06", "%s_five_continuation_bytes" % w, "a non-minimal integer with five continuation bytes is taken", "five",
             [feed([table, five[w]])], lambda sim: sim[0]["res"][0] == 2 and sim[0]["res"][6] == 0)
        case("06", "%s_six_continuation_bytes" % w, "a sixth continuation byte: ERR_INTEGER", "six", [feed([table, six[w]])],
             lambda sim: sim[0]["res"][0] == 1 and failed(sim[0], ERR_INTEGER, 3))
    top = (1 << 32) - 1
    forms = {"w7_indexed": (lambda v: indexed(v)), "w6_literal": (lambda v: literal(v, b"v")), "w4_literal": (lambda v: literal(v, b"v", mode=2)),
             "w4_never": (lambda v: literal(v, b"v", mode=3))}
    for name, f in forms.items():
        case("06", "%s_2p32m1" % name, "the index 2^32 - 1 is an integer, and no index: ERR_INDEX", "top", [feed([table, f(top)])],
             lambda sim: sim[0]["res"][0] == 1 and failed(sim[0], ERR_INDEX, 3) and sim[0]["facts"][1] == (1, 1, 0))
        case("06", "%s_2p32" % name, "2^32 is no integer: ERR_INTEGER", "over", [feed([table, f(top + 1)])],
             lambda sim: failed(sim[0], ERR_INTEGER, 3) and sim[0]["facts"][1] is None)
    case("06", "w7_length_2p32m1", "a string length of 2^32 - 1: ERR_TRUNCATED", "top", [feed([table, b"\x10" + enc_int(top, 7) + b"abc"])],
         lambda sim: failed(sim[0], ERR_TRUNCATED, 3))
    case("06", "w7_length_2p32", "a string length of 2^32: ERR_INTEGER", "over", [feed([table, b"\x10" + enc_int(top + 1, 7) + b"abc"])],
         lambda sim: failed(sim[0], ERR_INTEGER, 3))
    for setting in (4096, 65536):
        case("06", "w5_size_update_2p32m1_setting_%d" % setting, "a size update to 2^32 - 1: ERR_SIZE_UPDATE", "top",
             [feed([table, size_update(top) + indexed(2)])], lambda sim: failed(sim[0], ERR_SIZE_UPDATE, 3), setting=setting)
    case("06", "w5_size_update_2p32", "a size update to 2^32: ERR_INTEGER", "over", [feed([table, size_update(top + 1) + indexed(2)])],
         lambda sim: failed(sim[0], ERR_INTEGER, 3))
    for j, v in enumerate(BIG):
        case("06", "index_%d_indexed" % v, "the index %#x as an indexed field: ERR_INDEX (the bits above 2^24 are not the record's)" % v, "big_indexed" if v >> 24 else "clamp",
             [feed([table, indexed(2) + indexed(v)])], lambda sim: sim[0]["res"][:2] == (1, 70) and failed(sim[0], ERR_INDEX, 3))
        case("06", "index_%d_literal" % v, "the index %#x as a literal's name: ERR_INDEX" % v, "big_literal" if v >> 24 else "clamp",
             [feed([table, indexed(2) + literal(v, b"v", mode=1 + j % 3)])],
             lambda sim: sim[0]["res"][:2] == (1, 70) and failed(sim[0], ERR_INDEX, 3) and sim[0]["entries"] == 70)


# ---- family 7: Huffman alignments -------------------------------------------------------------------------------------------
def fam07():
    for k in range(8):
        strs = [b"0" * k + bytes([s]) for s in range(256)]
        for which in ("value", "name"):
            block = b"".join(literal(b"n", s, mode=3, hv=True) if which == "value" else literal(s, b"v", mode=3, hn=True) for s in strs)
            case("07", "every_byte_behind_%d_codes_as_%s" % (k, which), "every byte value behind %d five-bit codes, as never-indexed %ss: "
                 "codes of every length end at every bit" % (k, which), which, [feed([block])],
                 lambda sim, k=k: sim[0]["res"][:3] == (1, 256, 256 * (k + 2)) and sim[0]["res"][6] == 0)
        zeros = b"0" * k
        fillb = (-5 * k) % 8
        bad = [("eos_inside", bits(zeros, "E" + "00000" + "1" * ((-(5 * k + 35)) % 8))),
               ("eight_bits_of_padding", bits(zeros, "1" * (fillb + 8)))]
        if fillb:
            bad.append(("zero_bit_in_padding", bits(zeros, "1" * (fillb - 1) + "0")))
        for name, body in bad:
            case("07", "%s_behind_%d_codes" % (name, k), "%s behind %d five-bit codes: ERR_HUFFMAN" % (name.replace("_", " "), k), name,
                 [feed([literal(b"good", b"one", hv=True), b"\x10" + enc_str(b"n") + raw_huff(body)])],
                 lambda sim: sim[0]["res"][:2] == (1, 1) and failed(sim[0], ERR_HUFFMAN, 3) and sim[0]["entries"] == 1)


# ---- family 8: cuts and padding ------------------------------------------------------------------------------------------------
CUT_BLOCK = indexed(2) + literal(b"a", b"bc") + indexed(62)
CUT_WIRE = headers_frames(1, CUT_BLOCK, flags=1, cont=(2, 2), pad=3, priority=True)
# behind the frame header (the pad length not in), inside the priority bytes, inside the padding, between frames
CUT_PAIRS = ((9, 10), (9, 12), (12, 18), (18, 19), (18, 20), (20, 29), (9, 29), (29, 38), (19, 43))


def fam08():
    n = len(CUT_WIRE)
    done = lambda s: s["res"][:3] == (1, 3, 16) and s["res"][6] == 0 and s["blocks"][0][3] & 3 == 3  # noqa: E731
    for cut in range(1, n):
        case("08", "cut_at_%d" % cut, "a padded HEADERS frame with priority, an empty CONTINUATION and the closing one, cut at byte %d" % cut,
             "cut2", [("feed", [CUT_WIRE[:cut]]), ("feed", [CUT_WIRE[cut:]])],
             lambda sim, cut=cut: done(sim[1]) and sim[0]["res"][6] == (OPEN if cut >= 9 else 0) and sim[0]["res"][0] == 0)
    for a, b in CUT_PAIRS:
        case("08", "cut_at_%d_and_%d" % (a, b), "the same wire in three calls, cut at %d and %d" % (a, b), "cut3",
             [("feed", [CUT_WIRE[:a]]), ("feed", [CUT_WIRE[a:b]]), ("feed", [CUT_WIRE[b:]])],
             lambda sim: done(sim[2]) and sim[1]["res"][6] == OPEN and sim[2]["carried"])
    prio = b"\x80\x00\x00\x03\x10"
    for pr in (False, True):
        lo, fl = (6, 0x2c) if pr else (1, 0x0c)
        body = lambda pad, frag, padding: bytes([pad]) + (prio if pr else b"") + frag + bytes(padding)  # noqa: E731
        tag = "_priority" if pr else ""
        case("08", "pad_length_0" + tag, "PADDED with a pad length of 0", "pad", [("feed", [frame(1, fl, 1, body(0, b"\x82\x84", 0))])],
             lambda sim: sim[0]["res"][:2] == (1, 2) and sim[0]["res"][6] == 0)
        case("08", "pad_length_largest" + tag, "the pad length size - lo - 1, the largest legal: one fragment byte", "pad",
             [("feed", [frame(1, fl, 1, body(9, b"\x82", 9))])], lambda sim: sim[0]["res"][:2] == (1, 1) and sim[0]["closed"] == [b"\x82"])
        case("08", "pad_length_size_minus_lo" + tag, "the pad length size - lo: ERR_PADDING", "padbad",
             [("feed", [wire_of([b"\x82"]) + frame(1, fl, 3, body(10, b"", 10))])],
             lambda sim: sim[0]["res"][0] == 1 and failed(sim[0], ERR_PADDING, 3))
        case("08", "pad_length_255_short_frame" + tag, "a pad length of 255 on a frame of %d bytes: ERR_PADDING" % (lo + 2), "padbad",
             [("feed", [wire_of([b"\x82"]) + frame(1, fl, 3, body(255, b"\x82\x84", 0))])],
             lambda sim: sim[0]["res"][0] == 1 and failed(sim[0], ERR_PADDING, 3))
    block = literal(b"four", b"calls") + static_run(30) + indexed(62)
    w = headers_frames(1, block, cont=(7, 20), pad=5)
    case("08", "open_across_four_calls", "one block open across four calls", "four",
         [("feed", [w[:12]]), ("feed", [w[12:30]]), ("feed", [w[30:31]]), ("feed", [w[31:]])],
         lambda sim: [s["res"][6] for s in sim] == [OPEN, OPEN, OPEN, 0] and sim[3]["res"][:2] == (1, 32) and all(s["carried"] for s in sim[1:]))


# ---- family 9: index errors and the second pass ---------------------------------------------------------------------------------
def fam09():
    good9 = lambda j: literal(b"k", b"%d" % j) + indexed(62) * 8  # noqa: E731  (nine records)
    bad9 = literal(b"bad", b"x") + indexed(62) * 6 + indexed(300) + indexed(2)
    for k, blk, badb, per in ((0, good9, bad9, 9), (1, good9, bad9, 9), (57, good9, bad9, 9), (300, good9, bad9, 9),
                              (256, lambda j: literal(b"k", b"%d" % j) + indexed(62), literal(b"bad", b"x") + indexed(300), 2)):
        blocks = [blk(j) for j in range(k)] + [badb, blk(k + 1), blk(k + 2)]
        case("09", "index_error_in_block_%d_of_%d_records" % (k, per), "an index error in block %d, behind insertions in it and in the blocks "
             "in front: the table is the one behind block %d" % (k, k - 1), "index", [feed(blocks)],
             lambda sim, k=k, per=per: sim[0]["res"][0] == k and failed(sim[0], ERR_INDEX, 1 + 2 * k) and sim[0]["res"][3] == k
             and (not k or sim[0]["table"][0] == (b"k", b"%d" % (k - 1))) and len(sim[0]["nrec"]) == k + 1
             and next(i for i, s in enumerate(sim[0]["steps"]) if s[0] <= k < s[0] + max(1, s[1])) == k // min(THREADS, CHUNK // per))
    recs = [literal(b"r", b"%d" % j) if j % 97 == 0 else indexed(62) if j % 2 else indexed(2 + j % 60) for j in range(1300)]
    recs[1100] = indexed(400)
    case("09", "index_error_in_the_third_chunk", "an index error in record 1100 of a block of 1300", "chunk",
         [feed([literal(b"front", b"block"), b"".join(recs), indexed(62)])],
         lambda sim: sim[0]["res"][:2] == (1, 1) and failed(sim[0], ERR_INDEX, 3) and sim[0]["steps"][3] == (1, 0, 1024, 276) and sim[0]["entries"] == 1)
    trunc = indexed(2) + b"\x00\x05ab"
    index = literal(b"in", b"block") + indexed(99)
    okb = lambda j: literal(b"k", b"%d" % j) + indexed(62)  # noqa: E731
    case("09", "index_error_in_front_of_a_split_error", "an index error in block 1, a truncated string in block 2: the first decides", "both",
         [feed([okb(0), index, trunc, okb(3)])], lambda sim: sim[0]["res"][0] == 1 and failed(sim[0], ERR_INDEX, 3) and block_facts(trunc, 4096) is None and block_facts(index, 4096) == (2, 2, 0))
    case("09", "split_error_in_front_of_an_index_error", "a truncated string in block 1, an index error in block 2: the first decides", "both",
         [feed([okb(0), trunc, index, okb(3)])], lambda sim: sim[0]["res"][0] == 1 and failed(sim[0], ERR_TRUNCATED, 3) and sim[0]["facts"][1] is None)
    case("09", "index_error_in_an_insertions_name", "an inserting literal names an index that is none: the one thread that takes the record finds it",
         "insert", [feed([okb(0), okb(1) + literal(300, b"v") + indexed(62), okb(2)])],
         lambda sim: sim[0]["res"][0] == 1 and failed(sim[0], ERR_INDEX, 3) and split(sim[0]["closed"][1], 4096)[2][:2] == (1, 300)
         and sim[0]["table"][0] == (b"k", b"0"))
    case("09", "index_error_with_an_open_block_behind", "an index error in the last complete block, an open block behind it", "open",
         [("feed", [wire_of([okb(0), index]) + frame(1, 0, 5, indexed(2))]), ("feed", [frame(9, 4, 5, indexed(3))])],
         lambda sim: sim[0]["res"][0] == 1 and failed(sim[0], ERR_INDEX, 3) and not sim[1]["carried"] and sim[1]["res"][0] == 0)


# ---- family 10: caps ---------------------------------------------------------------------------------------------------------
def fam10():
    f1 = feed([b"".join(literal(b"k", b"%d" % j) for j in range(513)), indexed(62)])
    f4 = feed([b"".join(literal(b"", b"%d" % j) for j in range(RING + 52)), b"".join(indexed(62 + j) for j in range(100))])
    for name, f in (("513_insertions", f1), ("2100_insertions", f4)):
        for i, what in enumerate(("blocks", "fields", "string_bytes")):
            d = tuple(-1 if j == i else 0 for j in range(3))
            case("10", "%s_%s_cap" % (name, what), "the %s cap one short of what the call needs, then exactly that: the overflowing call "
                 "leaves everything untouched, its repeat is exact" % what.replace("_", " "), what,
                 [feed([literal(b"before", b"it")], 101), ("feed", f[1], f[2], ("need", d)), ("decode", ("need", (0, 0, 0)))],
                 lambda sim, i=i: sim[1]["res"][7] == 1 and sim[1]["rc"] and sim[1]["caps"][i] == sim[1]["res"][i] - 1 and sim[1]["entries"] == 1
                 and sim[2]["res"][7] == 0 and sim[2]["caps"] == sim[2]["res"][:3] and sim[2]["res"][:3] == sim[1]["res"][:3])


for _f in (fam01, fam02, fam03, fam04, fam05, fam06, fam07, fam08, fam09, fam10):
    _f()
_BY_ID = {c["id"]: c for c in CASES}


def by_id(cid):
    return _BY_ID[cid]


def check_cases():
    """every case's witness, from the model alone -> the cases"""
    same(len(_BY_ID), len(CASES), "case ids are unique")
    for c in CASES:
        same(bool(c["wit"](simulate(c))), True, "case %s reaches its edge (%s)" % (c["id"], c["edge"]))
    return CASES


def size_of(c):
    return sum(s.get("records", 0) for s in simulate(c))


def emu_subset():
    """the CPU suite's part: of every family and kind of edge the case with the fewest records, plus every case that
    caught a change of the mutation table alone"""
    best = {}
    for c in CASES:
        k = (c["fam"], c["key"])
        if k not in best or size_of(c) < size_of(best[k]):
            best[k] = c
    out = [c["id"] for c in CASES if best[(c["fam"], c["key"])] is c]
    return out + [t for t in CAUGHT_ALONE if t not in out]


def pin_sequence(c):
    """the case's block sequence, frames and cuts aside: [("block", bytes) | ("resize", n)]"""
    out = []
    for st, s in zip(c["steps"], simulate(c)):
        if st[0] == "resize":
            out.append(("resize", st[1]))
        elif s["res"][7] == 0:
            out += [("block", b) for b in s["closed"]]
    return out


# ---- the driver -----------------------------------------------------------------------------------------------------------------
def run_case(g, c):
    from tests.h2_hpack_lib import HH
    sim = simulate(c)
    h = HH(g, setting=c["setting"], max_block=c["max_block"], caps=c["caps"])
    for k, (st, s) in enumerate(zip(c["steps"], sim)):
        if st[0] == "resize":
            h.set_max_table_size(st[1])
            same(len(h.model.table.entries), s["entries"], "step %d: the harness's model against the case's" % k)
            continue
        if st[0] == "feed":
            _, res = h.feed(st[1], st[2] if len(st) > 2 else None, s["caps"])
        else:
            _, res = h.decode(s["caps"])
        same(res, s["res"], "step %d: the harness's model against the case's" % k)
    h.close()
