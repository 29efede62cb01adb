"""The send-window planner (k_h2_sw_plan, stage 4 of csrc/grdma_h2_sw_stage.inc, with h2sw_piece_size, h2sw_walk_piece and
h2sw_emit_piece of csrc/grdma_h2_sw.h) swept over message tables built from the constants it branches on: tile 64, plan
block 512, inlined slice 23 bytes, message header 5, frame header 9 (numbers: profiles/h2_send_plan_sweep.md).

A case is a deterministic script of framing calls (and real SETTINGS / WINDOW_UPDATE bytes between them) on one transport,
or one batch over a list of links.  The reference is tests/h2_send_model.SendModel; the drivers are SH.frame
(tests/h2_send_lib.py) and frame_batch (tests/h2_links_send_lib.py), which compare result block, progress, slice lengths
and table, wire image, inlined-slice pointers, header-arena bytes, windows, counters and the sentinels of an overflowing
call exactly.  Nothing here has a tolerance.

Every case names the edge it is there for, and a witness -- computed from the model alone (simulate) -- shows that the
case reaches it; check_cases() runs them all.  pytest rewrites no `assert` in a helper module: checks go through `same`."""
import collections
import functools

from oracle import pyorc
from tests.h2_device_lib import same
from tests.h2_send_lib import SH, body, settings, window_update
from tests.h2_send_model import (BLOCK, MAXW, STALL_CONN, STALL_STREAM, STALL_UNKNOWN, TILE, SendModel, back_fill, conn_end,
                                 frames_of, known, plan_facts, run_before, stream_end, tail_inlined, tile_lists)

FAMILIES = ("01", "02", "03", "04", "05", "06", "07", "08", "09", "10", "11", "12")
LENGTHS = (1, 63, 64, 65, 511, 512, 513, 1024, 1025, 4095, 4096)
UNKNOWN = 9999            # a stream no case opens
OPEN = dict(initial_window=MAXW, conn_window=MAXW)
FILLS = [14, 5, 19, 10, 1, 15, 6, 20]  # the back slice behind a run of 1 .. 8 empty messages
EMIT_WAVES = 1024         # H2SW_GRID * H2_EMIT_THREADS / 64 on the device: the emit's stride
# cases that were the only ones to catch a change of the mutation table (profiles/h2_send_plan_sweep.md)
CAUGHT_ALONE = []

CASES = []


def case(fam, name, edge, steps, wit, link=False, **kw):
    """steps: ("frame", msgs, progress or None, max_frame[, cap[, hdr_cap]]) with a cap as a number, None (what the call
    needs plus 8 slices) or ("need", d) (what it needs plus d); ("feed", bytes).  wit(sim) -> truth, sim = simulate(c).
    link: the case also runs through frame_windowed_batch, behind a neighbour link."""
    kw.setdefault("streams", (1, 3, 5))
    CASES.append(dict(id="%s_%s" % (fam, name), fam=fam, edge=edge, steps=steps, wit=wit, link=link, kw=kw, links=None))


def link_case(name, edge, links, wit):
    """links: [(SH keywords, msgs, progress or None, max_frame, cap, hdr_cap)], one framing call each, in one batch"""
    CASES.append(dict(id="11_%s" % name, fam="11", edge=edge, steps=None, wit=wit, link=True, kw=None, links=links))


def M(n, s=1, fl=0, seed=0):
    return (body(n, seed), s, fl)


def odd(k):
    return [2 * j + 1 for j in range(k)]


def slots_for(nstreams):
    t = 16
    while t < 2 * nstreams:
        t *= 2
    return t


# ---- the model alone ---------------------------------------------------------------------------------------------------
def _cap_of(spec, need, unit):
    if spec is None:
        return need + 8 * unit
    if isinstance(spec, tuple):
        return need + spec[1]
    return spec


def _sim_steps(kw, steps):
    streams = set(kw.get("streams", (1, 3, 5)))
    model = SendModel(kw.get("initial_window", 65535), kw.get("conn_window", 65535), kw.get("peer_max_frame", 16384))
    orc = pyorc.H2Parser(False)
    for s in sorted(streams):
        same(orc.open_stream(s), 0, "oracle open_stream(%d)" % s)
    out = []
    for st in steps:
        if st[0] == "feed":
            rc, ev = orc.feed(st[1])
            same(rc, 0, "the fed bytes' h2 error")
            out.append(dict(kind="feed", res=model.intake([e + (0,) for e in ev], [st[1]], 0, streams)))
            continue
        msgs, prog, mf = st[1], st[2] or [0] * len(st[1]), st[3]
        f = plan_facts(model, msgs, prog, mf, streams)
        probe = SendModel(model.iws, model.conn, model.pmf)
        probe.delta = dict(model.delta)
        lens, _, res, _ = probe.frame(msgs, prog, mf, 1 << 40, 1 << 40, streams)
        cap = _cap_of(st[4] if len(st) > 4 else None, len(lens), 1)
        hdr_cap = _cap_of(st[5] if len(st) > 5 else None, res[3], 32)
        lens, wire, res, after = model.frame(msgs, prog, mf, cap, hdr_cap, streams)
        out.append(dict(kind="frame", f=f, msgs=msgs, prog=prog, mf=mf, cap=cap, hdr_cap=hdr_cap, lens=lens, wire=wire, res=res,
                        after=after, need=(res[2], res[3])))
    return out


@functools.lru_cache(maxsize=None)
def _simulate(cid):
    c = by_id(cid)
    if c["links"] is not None:
        return [_sim_steps(kw, [("frame", msgs, prog, mf, cap, hdr_cap)])[0] for kw, msgs, prog, mf, cap, hdr_cap in c["links"]]
    return _sim_steps(c["kw"], c["steps"])


def simulate(c):
    """-> per step (per link of a link case) what the model alone says: the facts in front of a framing call
    (h2_send_model.plan_facts), the caps, and the call's result"""
    return _simulate(c["id"])


def frames(sim):
    return [s for s in sim if s["kind"] == "frame"]


# ---- witness parts -------------------------------------------------------------------------------------------------------
def next_of_stream_gets_nothing(f, i):
    later = [j for j in range(i + 1, f["n"]) if f["streams"][j] == f["streams"][i]]
    return not later or f["g"][later[0]] == 0


def blocks_of(f, s):
    return sorted({i // BLOCK for i in range(f["n"]) if f["streams"][i] == s})


def tiles_of(f, s):
    return sorted({i // TILE for i in range(f["n"]) if f["streams"][i] == s})


# ---- family 1: table length ------------------------------------------------------------------------------------------------
def fam01():
    for n in LENGTHS:
        for per in ("one", "each"):
            ids = [1] * n if per == "one" else odd(n)
            msgs = [M(10, s, 0, i) for i, s in enumerate(ids)]
            kw = dict(streams=tuple(sorted(set(ids))), table_slots=slots_for(len(set(ids))))
            case("01", "n%d_%s_open" % (n, per), "%d messages, %s, windows open" % (n, per), [("frame", msgs, None, 16384)],
                 lambda sim, n=n: sim[0]["f"]["n"] == n and sim[0]["res"][:2] == (n, 0) and sim[0]["res"][6] == 0,
                 link=(n == 1 and per == "one"), **kw, **OPEN)
            w = 15 * (n - 1) + 7
            if per == "one":
                case("01", "n%d_one_binds" % n, "%d messages, the stream's window ends inside the last" % n,
                     [("frame", msgs, None, 16384)],
                     lambda sim, n=n: stream_end(sim[0]["f"], 1) == (n - 1, 7) and sim[0]["res"][6] == STALL_STREAM,
                     **kw, initial_window=w, conn_window=MAXW)
            else:
                case("01", "n%d_each_binds" % n, "%d messages, the connection's window ends inside the last" % n,
                     [("frame", msgs, None, 16384)],
                     lambda sim, n=n: conn_end(sim[0]["f"]) == (n - 1, 7) and sim[0]["res"][6] == STALL_CONN,
                     **kw, initial_window=MAXW, conn_window=w)


# ---- family 2: where a window ends -----------------------------------------------------------------------------------------
def fam02():
    for idx in (0, 62, 63, 64, 65, 511, 512, 513, "last"):
        n = 70 if idx != "last" and idx <= 65 else 600
        i = n - 1 if idx == "last" else idx
        for cut in (15, 14, 1, 2, 3, 4, 5, 6):
            w = 15 * i + cut
            what = "exactly at its end" if cut == 15 else "at byte %d" % cut
            msgs = [M(10, 1, 2 * (j & 1), j) for j in range(n)]
            case("02", "stream_m%s_cut%d" % (idx, cut), "the stream's window ends in message %d %s" % (i, what),
                 [("frame", msgs, None, 16384)],
                 lambda sim, i=i, cut=cut: stream_end(sim[0]["f"], 1) == (i, cut) and next_of_stream_gets_nothing(sim[0]["f"], i)
                 and sim[0]["f"]["g"][i] == cut, link=(idx == 0 and cut == 15), initial_window=w, conn_window=MAXW)
            msgs = [M(10, (1, 3, 5)[j % 3], 2 * (j & 1), j) for j in range(n)]
            exact_block = (i == 511 and cut == 15)
            case("02", "conn_m%s_cut%d" % (idx, cut), "the connection's window ends in message %d %s%s" % (
                 i, what, ": the stream-allowed bytes of block 0 are the window exactly (base_a)" if exact_block else ""),
                 [("frame", msgs, None, 16384)],
                 lambda sim, i=i, cut=cut, eb=exact_block: conn_end(sim[0]["f"]) == (i, cut) and sim[0]["f"]["g"][i] == cut
                 and all(x == 0 for x in sim[0]["f"]["g"][i + 1:])
                 and (not eb or sum(sim[0]["f"]["a"][:BLOCK]) == sim[0]["f"]["conn"]), initial_window=MAXW, conn_window=w)


# ---- family 3: distinct streams per tile --------------------------------------------------------------------------------------
def _rotation(n, ids, target, big=40, small=1):
    return [M(big if ids[i % len(ids)] == target else small, ids[i % len(ids)], 0, i) for i in range(n)]


def fam03():
    for k, entries in ((1, (0,)), (2, (0, 1)), (3, (0, 1, 2)), (63, (0, 1, 2, 62)), (64, (0, 1, 2, 63))):
        ids = odd(k)
        last = {ids[i % k]: i for i in range(TILE)}
        order = sorted(last, key=last.get)  # tile 0's list
        for e in entries:
            target = order[e]
            msgs = _rotation(192, ids, target)
            w = sum(5 + len(b) for b, s, _ in msgs[:128] if s == target) + 10

            def wit(sim, k=k, e=e, target=target, ids=ids):
                f = sim[0]["f"]
                lists = tile_lists(f)
                end = stream_end(f, target)
                return (all(len(t) == k for t in lists) and lists[0][e] == target and target in lists[1]
                        and end is not None and end[0] // TILE == 2 and 0 < f["a"][end[0]] < f["rem"][end[0]]
                        and all(stream_end(f, s) is None for s in ids if s != target))
            case("03", "k%d_entry%d_binds_in_tile2" % (k, e),
                 "%d distinct streams a tile; stream %d is entry %d of tile 0's list and binds in tile 2" % (k, target, e),
                 [("frame", msgs, None, 16384)], wit, link=True, streams=tuple(ids), table_slots=slots_for(k),
                 initial_window=w, conn_window=MAXW)
    ids = (1, 3, 5)
    msgs = _rotation(512, ids, 1)
    w = sum(5 + len(b) for b, s, _ in msgs[:448] if s == 1) + 10
    case("03", "every_tile_of_a_block", "stream 1 in every tile of a block among two others, its window ends in tile 7",
         [("frame", msgs, None, 16384)],
         lambda sim: tiles_of(sim[0]["f"], 1) == list(range(8)) and stream_end(sim[0]["f"], 1)[0] // TILE == 7,
         initial_window=w, conn_window=MAXW)
    for name, lanes in (("lane0", (0,)), ("lane63", (63,)), ("among", (10, 20, 33)), ("whole_tile", tuple(range(64)))):
        msgs = [M(10, UNKNOWN if (i // TILE == 1 and i % TILE in lanes) else 1, 0, i) for i in range(192)]
        w = 15 * sum(1 for _, s, _ in msgs[:130] if s == 1) + 7

        def wit(sim, lanes=lanes):
            f = sim[0]["f"]
            return ([i for i in range(f["n"]) if not known(f, i)] == [64 + x for x in lanes]
                    and (tile_lists(f)[1] == []) == (len(lanes) == 64) and stream_end(f, 1)[0] == 130
                    and sim[0]["res"][6] == STALL_STREAM | STALL_UNKNOWN)
        case("03", "unknown_%s" % name, "a stream the map does not hold in tile 1 (%s); stream 1 binds behind it in tile 2" % name,
             [("frame", msgs, None, 16384)], wit, streams=(1,), initial_window=w, conn_window=MAXW)


# ---- family 4: hand-over across blocks -------------------------------------------------------------------------------------
def _placed(n, at, big=40):
    """stream 1 everywhere with small messages, stream 3 with big ones at the indices `at`"""
    return [M(big, 3, 0, i) if i in at else M(1, 1, 0, i) for i in range(n)]


def fam04():
    def ends(at_last, blocks=None, tiles=None):
        def wit(sim):
            f = frames(sim)[0]["f"]
            end = stream_end(f, 3)
            return (end is not None and end[0] == at_last and 0 < f["a"][at_last] < f["rem"][at_last] and stream_end(f, 1) is None
                    and (blocks is None or blocks_of(f, 3) == blocks) and (tiles is None or tiles_of(f, 3) == tiles))
        return wit
    for name, edge, n, at, blocks, tiles in (
            ("b_b1_through_511_512", "stream 3 at 511 and 512: blocks 0 and 1", 600, (511, 512), [0, 1], [7, 8]),
            ("b_b2_not_b1", "stream 3 in blocks 0 and 2, not in 1", 1100, (100, 1030), [0, 2], None),
            ("first_and_last_tile", "stream 3 in tiles 0 and 7 of block 0 only (`later` across seven tiles), binds in block 1",
             600, (5, 500, 520), [0, 1], [0, 7, 8]),
            ("last_tile_then_first", "stream 3 in the last tile of block 0 and the first of block 1", 600, (510, 515), [0, 1], [7, 8]),
            ("neighbour_tiles", "stream 3 in tiles 2 and 3 of block 0, binds in block 1", 600, (130, 200, 520), [0, 1], [2, 3, 8]),
            ("three_blocks", "stream 3 in blocks 0, 1 and 2, binds in block 2", 1100, (10, 600, 1030), [0, 1, 2], None)):
        case("04", name, edge + "; its window ends in message %d" % at[-1],
             [("feed", window_update(1, 1 << 20)), ("frame", _placed(n, at), None, 16384)],
             ends(at[-1], blocks, tiles), streams=(1, 3), initial_window=45 * (len(at) - 1) + 10, conn_window=MAXW)
    ids = (1, 33, 65, 97)
    msgs = [M(10, ids[i % 4], 0, i) for i in range(512)]

    def wit(sim):
        f = sim[0]["f"]
        return (len({(s >> 1) & 15 for s in ids}) == 1 and all(sorted(t) == list(ids) for t in tile_lists(f)) and len(tile_lists(f)) == 8
                and all(stream_end(f, s)[0] // TILE == 7 for s in ids))
    case("04", "eight_tiles_claim_a_new_slot", "eight tiles name the same four new streams at once; 16 slots, ids colliding on slot 0",
         [("frame", msgs, None, 16384)], wit, streams=ids, table_slots=16, initial_window=15 * 120 + 7, conn_window=MAXW)


# ---- family 5: windows at 0, negative, both stalls on one message ---------------------------------------------------------------
def fam05():
    three = [M(30, 1), M(10, 3, 2), M(4, 5)]
    case("05", "stream_window_0", "a stream window of exactly 0", [("frame", three, None, 16)],
         lambda sim: sim[0]["f"]["windows"][1] == 0 and sim[0]["res"][5:7] == (0, STALL_STREAM) and sim[0]["f"]["pieces"] == [],
         initial_window=0, conn_window=1000)
    case("05", "conn_window_0", "a connection window of exactly 0", [("frame", three, None, 16)],
         lambda sim: sim[0]["f"]["conn"] == 0 and sim[0]["res"][5:7] == (0, STALL_CONN), initial_window=1000, conn_window=0)
    case("05", "unknown_alone", "STALL_UNKNOWN alone: every message on a stream the map does not hold",
         [("frame", [M(30, UNKNOWN), M(3, UNKNOWN)], None, 16)],
         lambda sim: sim[0]["res"][5:7] == (0, STALL_UNKNOWN) and sim[0]["res"][1] == 2, **OPEN)
    case("05", "both_stalls_on_one_message", "one message with a < r and g < a", [("frame", [M(30, 1)], None, 16)],
         lambda sim: sim[0]["f"]["g"][0] < sim[0]["f"]["a"][0] < sim[0]["f"]["rem"][0] and sim[0]["res"][6] == STALL_CONN | STALL_STREAM,
         initial_window=20, conn_window=10)
    case("05", "all_three_stalls", "all three stall bits in one call", [("frame", [M(30, 1), M(9, UNKNOWN), M(30, 3)], None, 16)],
         lambda sim: sim[0]["res"][6] == 7 and sim[0]["f"]["g"] == [20, 0, 5], initial_window=20, conn_window=25)
    neg = [M(200, 1, 2)]
    case("05", "negative_stream_window", "INITIAL_WINDOW_SIZE lowered through SETTINGS below what is in flight: delta negative",
         [("frame", neg, None, 64), ("feed", settings([(4, 30)])), ("frame", neg + [M(5, 3)], [100, 0], 64),
          ("feed", window_update(1, 71)), ("frame", neg, [100], 64)],
         lambda sim: sim[0]["after"] == [100] and sim[2]["f"]["windows"] == {1: -70, 3: 30} and sim[2]["f"]["g"] == [0, 10]
         and sim[4]["f"]["windows"][1] == 1 and sim[4]["f"]["g"] == [1], link=True, initial_window=100, conn_window=1000)
    msgs = [M(10, 1, 0, i) for i in range(600)]
    case("05", "negative_window_over_two_blocks", "a negative stream window under 600 messages: nothing granted in either block",
         [("frame", [M(200, 1)], None, 64), ("feed", settings([(4, 30)])), ("frame", msgs, None, 64)],
         lambda sim: sim[2]["f"]["windows"][1] == -70 and sim[2]["res"][5:7] == (0, STALL_STREAM) and sim[2]["f"]["n"] > BLOCK,
         streams=(1,), initial_window=100, conn_window=1000)


# ---- family 6: compaction ----------------------------------------------------------------------------------------------------
def fam06():
    msgs = [M(10, (1, UNKNOWN, 3)[i % 3], 0, i) for i in range(200)]
    case("06", "granted_among_nothing", "every third message granted nothing: piece index differs from message index",
         [("frame", msgs, None, 16384)],
         lambda sim: [i for i, _, _ in sim[0]["f"]["pieces"]] == [i for i in range(200) if i % 3 != 1], link=True, **OPEN)
    blocked = [M(100, 3, 0, 0)] + [M(10, (1, 3)[i % 2], 0, i) for i in range(1, 100)]
    case("06", "held_behind_an_unfinished_message", "stream 3 held behind its unfinished first message among stream 1's pieces",
         [("feed", window_update(1, 1 << 20)), ("frame", blocked, None, 16384)],
         lambda sim: [i for i, _, _ in sim[1]["f"]["pieces"]] == [0] + list(range(2, 100, 2)), initial_window=50, conn_window=MAXW)
    for kept in (511, 512, 513):
        msgs = [M(10, 1 if (i % 2 == 0 and i < 2 * kept) else UNKNOWN, 0, i) for i in range(1100)]
        case("06", "kept%d_of_1100" % kept, "%d pieces out of 1100 messages: the size loop's own blocks" % kept,
             [("frame", msgs, None, 16384)], lambda sim, kept=kept: len(sim[0]["f"]["pieces"]) == kept and sim[0]["f"]["n"] == 1100,
             streams=(1,), **OPEN)


# ---- family 7: runs of header-only pieces ---------------------------------------------------------------------------------------
def _run_wit(first, length, fill=None, fits=None, follower=True):
    def wit(sim):
        f = sim[0]["f"]
        k = first + length
        ok = all(tail_inlined(p) for p in f["pieces"][first:k]) and (first == 0 or not tail_inlined(f["pieces"][first - 1]))
        if not follower:
            return ok and len(f["pieces"]) == k
        ok = ok and not tail_inlined(f["pieces"][k]) and run_before(f, k) == length
        if fill is not None:
            ok = ok and back_fill(f, k) == fill
        if fits is not None:
            ok = ok and (back_fill(f, k) + 9 <= 23) == fits
        return ok
    return wit


def fam07():
    empty = M(0, 1)
    for L in (1, 2, 3, 4, 5, 6, 7, 8, 63, 64, 65, 513, 1025):
        fill = FILLS[L - 1] if L <= 8 else None
        fits = None if fill is None else fill + 9 <= 23
        case("07", "empty%d_front_plain" % L, "a run of %d empty messages at piece 0, then a plain piece%s" % (
             L, "" if fill is None else "; the back slice holds %d: its frame header %s" % (fill, "fits" if fits else "does not fit")),
             [("frame", [empty] * L + [M(10, 1, 2, 7)], None, 16384)], _run_wit(0, L, fill, fits), link=L <= 8, **OPEN)
    for L in range(1, 9):
        fill = FILLS[L - 1]
        case("07", "empty%d_middle_other_stream" % L, "plain, a run of %d, a piece of another stream (back slice %d)" % (L, fill),
             [("frame", [M(10, 1, 0, 3)] + [empty] * L + [M(10, 3, 0, 7)], None, 16384)], _run_wit(1, L, fill), **OPEN)
        case("07", "empty%d_end" % L, "plain, then a run of %d at the table's end" % L,
             [("frame", [M(10, 1, 0, 3)] + [empty] * L, None, 16384)], _run_wit(1, L, follower=False), **OPEN)
        p = 1 + (L - 1) % 4
        case("07", "empty%d_front_resumed_p%d" % (L, p), "a run of %d, then a resumed piece with p = %d (back slice %d)" % (L, p, fill),
             [("frame", [empty] * L + [M(10, 3, 2, 7)], [0] * L + [p], 16384)], _run_wit(0, L, fill), **OPEN)
        case("07", "empty%d_front_two_frames" % L, "a run of %d, then a piece of two frames (mf 8, back slice %d)" % (L, fill),
             [("frame", [empty] * L + [M(10, 1, 2, 7)], None, 8)], _run_wit(0, L), **OPEN)
    for cut in (1, 2, 3, 4, 5):
        for L in (1, 2, 3, 8):
            ids = odd(L + 1)
            msgs = [M(10, s, 0, s) for s in ids]
            # (the follower resumes at p = 5: whatever it is granted lies behind the header)
            case("07", "cut%d_run%d_then_resumed" % (cut, L),
                 "%d grants that end at byte %d of the header (one stream each), then a piece resumed behind the header" % (L, cut),
                 [("frame", msgs, [0] * L + [5], 16384)], _run_wit(0, L), streams=tuple(ids), table_slots=slots_for(L + 1),
                 initial_window=cut, conn_window=MAXW)
    for L in (8, 9):
        msgs = [M(10, 1, 0, i) for i in range(508)] + [empty] * L + [M(10, 1, 2, 9)] + [M(10, 1, 0, i) for i in range(40)]
        case("07", "empty%d_across_piece_511_512" % L, "a run of %d from piece 508 on: it crosses piece 511 / 512" % L,
             [("frame", msgs, None, 16384)], _run_wit(508, L), streams=(1,), **OPEN)


# ---- family 8: frame sizes ------------------------------------------------------------------------------------------------------
def fam08():
    msgs = [M(10, 1, 2, 1), M(10, 3, 1, 2), M(10, 5, 3, 3)]
    for mf in (1, 4, 5, 6, 7, 14, 15, 16):
        case("08", "mf%d" % mf, "frames of %d bytes under pieces of 15 (g = 15)" % mf, [("frame", msgs, None, mf)],
             lambda sim, mf=mf: sim[0]["f"]["mf"] == mf and [g for _, _, g in sim[0]["f"]["pieces"]] == [15] * 3,
             link=(mf == 1), **OPEN)
    for F in (63, 64, 65, 128, 129):
        case("08", "piece_of_%d_frames" % F, "a piece of %d frames of 7 bytes: the emit's lane stride" % F,
             [("frame", [M(7 * F - 5, 1, 2, F), M(3, 3, 0, 1)], None, 7)],
             lambda sim, F=F: frames_of(sim[0]["f"], 0) == F and sim[0]["f"]["pieces"][0][2] == 7 * F, **OPEN)
    big = [M(16384 + 16385 - 5, 1, 2, 5)]
    case("08", "peer_max_frame_binds", "min(max_frame, peer MAX_FRAME_SIZE): the peer's 16384 below the call's 16385",
         [("frame", big, None, 16385)], lambda sim: sim[0]["f"]["mf"] == 16384 and frames_of(sim[0]["f"], 0) == 3,
         peer_max_frame=16384, **OPEN)
    case("08", "call_max_frame_binds", "min(max_frame, peer MAX_FRAME_SIZE): the call's 16384 below the peer's 16385",
         [("frame", big, None, 16384)], lambda sim: sim[0]["f"]["mf"] == 16384 and frames_of(sim[0]["f"], 0) == 3,
         peer_max_frame=16385, **OPEN)

    def end_stream_bits(sim, step=0):
        wire, out, at = sim[step]["wire"], [], 0
        while at < len(wire):
            out.append(wire[at + 4])
            at += 9 + int.from_bytes(wire[at:at + 3], "big")
        return out
    for p in (3, 5, 7):
        case("08", "finished_in_a_resumed_piece_p%d" % p, "a message with END_STREAM finished in a piece resumed at %d (`whole`)" % p,
             [("frame", [M(10, 1, 2, 1), M(10, 3, 3, 2)], [p, 0], 4)],
             lambda sim, p=p: end_stream_bits(sim)[:-(-(15 - p) // 4)] == [0] * (-(-(15 - p) // 4) - 1) + [1]
             and end_stream_bits(sim)[-1] == 1 and sum(end_stream_bits(sim)) == 2, **OPEN)
    case("08", "end_stream_held_by_the_window",
         "a message with END_STREAM cut by its window: no frame carries the flag; the next call's last does",
         [("frame", [M(10, 1, 2, 1)], None, 4), ("feed", window_update(1, 100)), ("frame", [M(10, 1, 2, 1)], [9], 4)],
         lambda sim: sum(end_stream_bits(sim)) == 0 and end_stream_bits(sim, 2) == [0, 1], initial_window=9, conn_window=MAXW)
    case("08", "compressed_flag", "the compressed flag in the message header, alone and beside END_STREAM",
         [("frame", [M(10, 1, 1, 1), M(0, 3, 3, 2), M(10, 5, 0, 3)], None, 16384)],
         lambda sim: [sim[0]["wire"][9], sim[0]["wire"][9 + 15 + 9], sim[0]["wire"][9 + 15 + 9 + 5 + 9]] == [1, 1, 0], **OPEN)


# ---- family 9: caps -------------------------------------------------------------------------------------------------------------
def fam09():
    msgs = [M(0 if i % 7 == 3 else 10, 1, 0, i) for i in range(600)]
    w = sum(5 + len(b) for b, _, _ in msgs[:550]) + 7
    kw = dict(streams=(1,), initial_window=w, conn_window=MAXW)
    exact = ("frame", msgs, None, 16384, ("need", 0), ("need", 0))

    def wit(first_over):
        def w_(sim):
            fr = frames(sim)
            return ([s["res"][7] for s in fr] == ([1] if first_over else []) + [0] and fr[0]["f"]["n"] > BLOCK
                    and fr[-1]["cap"] == fr[-1]["need"][0] and fr[-1]["hdr_cap"] == fr[-1]["need"][1]
                    and fr[0]["need"] == fr[-1]["need"] and stream_end(fr[-1]["f"], 1)[0] == 550)
        return w_
    case("09", "exactly_what_the_call_needs", "slice cap and header cap exactly what 600 messages need", [exact], wit(False),
         link=True, **kw)
    case("09", "one_slice_less_then_exact", "the slice cap one short: nothing written, scratch words back at 0; the next call is exact",
         [("frame", msgs, None, 16384, ("need", -1), ("need", 0)), exact], wit(True), link=True, **kw)
    case("09", "32_header_bytes_less_then_exact", "the header cap 32 bytes short, then exact",
         [("frame", msgs, None, 16384, ("need", 0), ("need", -32)), exact], wit(True), link=True, **kw)


# ---- family 10: two calls in a row ------------------------------------------------------------------------------------------------
def fam10():
    one = [M(10, (1, 3, 5)[i % 3], 0, i) for i in range(1100)]  # (367, 367 and 366 messages)
    two = [M(10, (3, 7, 9)[i % 3], 0, i) for i in range(90)]
    three = [M(10, (1, 5, 3)[i % 3], 0, i) for i in range(90)]
    # no intake between the calls: an intake moves the entries into the second table and would clear the words itself
    w = 15 * 367 + 100

    def wit(sim):
        f1, f2, f3 = (s["f"] for s in sim)
        return (all(s["kind"] == "frame" for s in sim) and all(blocks_of(f1, s) == [0, 1, 2] for s in (1, 3, 5))
                and sim[0]["res"][:2] == (1100, 0) and f2["windows"] == {3: 100, 7: w, 9: w} and stream_end(f2, 3) == (18, 10)
                and stream_end(f2, 7) is None and (f3["windows"][1], f3["windows"][5], f3["windows"][3]) == (100, 115, 0)
                and stream_end(f3, 1) == (18, 10) and stream_end(f3, 5) == (22, 10))
    case("10", "scratch_words_reset_between_calls",
         "call 1: three streams over three blocks; call 2, no intake between, names one of them and two new ones; call 3 the two "
         "call 2 left out",
         [("frame", one, None, 16384), ("frame", two, None, 16384), ("frame", three, None, 16384)], wit, link=True,
         streams=(1, 3, 5, 7, 9), initial_window=w, conn_window=MAXW)
    wb = 15 * 300 + 7

    def wit_b(sim):
        f1, f2, f3 = (s["f"] for s in frames(sim))
        return (sim[0]["res"][6] == STALL_STREAM and all(stream_end(f1, s)[0] // BLOCK == 1 for s in (1, 3, 5))
                and f2["windows"] == {3: 100, 7: wb, 9: wb} and stream_end(f2, 3) == (18, 10)
                and f3["windows"][1] == f3["windows"][5] == 100 and stream_end(f3, 1) == (18, 10) and stream_end(f3, 3)[1] == 0)
    case("10", "calls_in_a_row_behind_an_intake",
         "call 1: three streams over three blocks, all bind in block 1; WINDOW_UPDATEs; call 2 names one of them and two new ones; "
         "call 3 the others",
         [("frame", one, None, 16384), ("feed", b"".join(window_update(s, 100) for s in (1, 3, 5))),
          ("frame", two, None, 16384), ("frame", three, None, 16384)], wit_b, streams=(1, 3, 5, 7, 9),
         initial_window=wb, conn_window=MAXW)


# ---- family 11: the link path ---------------------------------------------------------------------------------------------------
LK = dict(streams=(1, 3), table_slots=16)


def _link(kind, seed=0):
    """one link's call by kind -> (SH keywords, msgs, progress, max_frame, cap, hdr_cap)"""
    if kind == "none":      # no pieces: the connection's window is 0
        return (dict(LK, conn_window=0), [M(10, 1, 0, seed)], None, 64, None, None)
    if kind == "plain":
        return (dict(LK), [M(10, 1, 0, seed), M(30, 3, 2, seed + 1), M(4, 1, 1, seed + 2)], None, 16, None, None)
    if kind == "run_end":   # the last piece header-only
        return (dict(LK), [M(10, 1, 0, seed), M(0, 3, 0), M(0, 1, 0)], None, 64, None, None)
    if kind == "run_front":
        return (dict(LK), [M(0, 1, 0), M(0, 1, 0), M(10, 3, 2, seed)], None, 64, None, None)
    if kind == "bound":     # the stream's window ends inside the second message
        return (dict(LK, initial_window=22), [M(10, 1, 0, seed), M(10, 1, 0, seed + 1), M(10, 3, 0, seed + 2)], None, 64, None, None)
    if kind == "overflow":
        return (dict(LK), [M(10, 1, 0, seed), M(30, 3, 2, seed + 1)], None, 16, ("need", -1), None)
    if isinstance(kind, int):  # `kind` pieces, every seventh header-only
        return (dict(streams=(1,), table_slots=16, **OPEN), [M(0 if i % 7 == 3 else 10, 1, 0, i) for i in range(kind)], None, 16384,
                None, None)
    raise ValueError(kind)


def fam11():
    def npieces(sim):
        return [0 if s["res"][7] else len(s["f"]["pieces"]) for s in sim]
    rot = ("plain", "none", "run_end", "run_front", "bound")
    for L in (1, 2, 64, 65, 256):
        kinds = [rot[l % 5] for l in range(L)] if L > 2 else (["run_end"], ["run_end", "run_front"])[L - 1]
        link_case("L%d" % L, "%d links by rotation of %s" % (L, "/".join(dict.fromkeys(kinds))), [_link(k, l) for l, k in enumerate(kinds)],
                  lambda sim, L=L: len(sim) == L and all(s["res"][7] == 0 for s in sim))
    for name, kinds in (("none_front", ("none", "plain", "plain")), ("none_middle", ("plain", "none", "none", "plain")),
                        ("none_back", ("plain", "plain", "none")), ("all_but_one_none", ("none", "none", "plain", "none", "none"))):
        link_case(name, "links without pieces: " + name, [_link(k, l) for l, k in enumerate(kinds)],
                  lambda sim, kinds=kinds: [n == 0 for n in npieces(sim)] == [k == "none" for k in kinds])
    link_case("overflow_between_framed", "an overflowed link between two framed ones",
              [_link(k, l) for l, k in enumerate(("plain", "overflow", "run_front"))], lambda sim: [s["res"][7] for s in sim] == [0, 1, 0])
    link_case("header_only_last_then_next_link", "the last piece of link 0 is header-only; link 1's first piece must not merge into it",
              [_link("run_end"), _link("plain", 5)],
              lambda sim: tail_inlined(sim[0]["f"]["pieces"][-1]) and sim[1]["lens"][0] == 14)
    link_case("stride_wraps_inside_and_across",
              "pieces 1000 + 100 + 1100: the emit's stride of %d wraps across a link boundary and inside a link" % EMIT_WAVES,
              [_link(1000), _link(100), _link(1100)],
              lambda sim: npieces(sim) == [1000, 100, 1100] and 1000 <= EMIT_WAVES < 1100 and 1100 + EMIT_WAVES < 2200)


# ---- family 12: the intake's grid stride (hardware only) ----------------------------------------------------------------------------
INTAKE_IDS = (1, 33, 65, 97)
INTAKE_FRAMES = 32800


def intake_slices():
    ids = (0,) + INTAKE_IDS
    frames_ = [window_update(ids[j % 5], 1 + j % 3) for j in range(INTAKE_FRAMES)]
    per = 1024
    return [b"".join(frames_[k:k + per]) for k in range(0, INTAKE_FRAMES, per)]


def fam12():
    CASES.append(dict(id="12_intake_of_65600_events", fam="12", steps=None, links=None, link=False, kw=None,
                      edge="WINDOW_UPDATE frames for %d events: k_h2_sw_take's 65536 threads take their grid stride" % (2 * INTAKE_FRAMES),
                      wit=lambda sim: 2 * INTAKE_FRAMES >= 65537 and sum(len(s) for s in intake_slices()) == 13 * INTAKE_FRAMES))


for _f in (fam01, fam02, fam03, fam04, fam05, fam06, fam07, fam08, fam09, fam10, fam11, fam12):
    _f()
_BY_ID = {c["id"]: c for c in CASES}


def by_id(cid):
    return _BY_ID[cid]


def paths_of(c):
    if c["fam"] == "11":
        return ("link",)
    return ("single", "link") if c["link"] else ("single",)


def tests():
    return [(c["id"], p) for c in CASES for p in paths_of(c)]


def check_cases():
    """every case's witness, from the model alone -> the cases"""
    same(len(_BY_ID), len(CASES), "case ids are unique")
    for c in CASES:
        sim = None if c["fam"] == "12" else simulate(c)
        same(bool(c["wit"](sim)), True, "case %s reaches its edge (%s)" % (c["id"], c["edge"]))
    # family 7 as a whole: the back slice walks through FILLS, and followers that fit and that do not both occur
    fits = collections.Counter()
    for L in range(1, 9):
        f = simulate(by_id("07_empty%d_front_plain" % L))[0]["f"]
        same(back_fill(f, L), FILLS[L - 1], "back slice behind a run of %d" % L)
        fits[back_fill(f, L) + 9 <= 23] += 1
    same(sorted(fits), [False, True], "followers that fit the back slice and that do not")
    return CASES


def size_of(c):
    if c["fam"] == "12":
        return 2 * INTAKE_FRAMES
    if c["links"] is not None:
        return sum(len(l[1]) for l in c["links"])
    return sum(len(s[1]) for s in c["steps"] if s[0] == "frame")


def emu_subset():
    """the CPU suite's part: of every family but 12 (hardware only) the smallest case, on every path it runs on, plus every
    test that caught a mutation alone"""
    out = []
    for fam in FAMILIES[:-1]:
        c = min((c for c in CASES if c["fam"] == fam), key=lambda c: (size_of(c), CASES.index(c)))
        out += [(c["id"], p) for p in paths_of(c)]
    return out + [t for t in CAUGHT_ALONE if t not in out]


# ---- the driver -----------------------------------------------------------------------------------------------------------------
def _neighbour_call(step):
    """the link in front of a case on the link path: it ends with a header-only piece, which nothing of the case's link
    may merge into"""
    return ([M(10, 1, 0, step), M(0, 1, 0)], [0, 0], 64)


def run_case(g, c, path):
    from tests import h2_links_send_lib as LL
    if c["fam"] == "12":
        return run_intake(g)
    sim = simulate(c)
    if c["links"] is not None:
        hs = [SH(g, **kw) for kw, _, _, _, _, _ in c["links"]]
        calls = {l: (s["msgs"], s["prog"], s["mf"], s["cap"], s["hdr_cap"]) for l, s in enumerate(sim)}
        got = LL.frame_batch(hs, list(range(len(hs))), calls)
        for l, s in enumerate(sim):
            same(got[l], (s["lens"], s["wire"], s["res"], s["after"]), "link %d: the harness's model against the case's" % l)
        for h in hs:
            h.close()
        return
    h = SH(g, **c["kw"])
    front = SH(g, streams=(1,), table_slots=16, **OPEN) if path == "link" else None
    for k, s in enumerate(sim):
        if s["kind"] == "feed":
            same(h.feed([c["steps"][k][1]]), s["res"], "step %d: intake" % k)
        elif path == "single":
            got = h.frame(s["msgs"], s["prog"], s["mf"], cap=s["cap"], hdr_cap=s["hdr_cap"])
            same(got, (s["wire"], s["res"], s["after"]), "step %d: the harness's model against the case's" % k)
        else:
            got = LL.frame_batch([front, h], [0, 1], {0: _neighbour_call(k), 1: (s["msgs"], s["prog"], s["mf"], s["cap"], s["hdr_cap"])})
            same(got[1], (s["lens"], s["wire"], s["res"], s["after"]), "step %d: the harness's model against the case's" % k)
    h.close()
    if front:
        front.close()


def run_intake(g):
    h = SH(g, streams=INTAKE_IDS, table_slots=16)
    slices = intake_slices()
    res = h.feed(slices, ev_cap=2 * INTAKE_FRAMES + 4096)
    same(res[0], INTAKE_FRAMES, "WINDOW_UPDATE frames applied")
    same(res[4], 0, "violations")
    h.close()
