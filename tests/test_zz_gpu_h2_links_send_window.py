"""Send flow control on many links: grdma_h2_sw_intake_batch and grdma_h2_sw_frame_batch (the five k_h2_links_sw_*
kernels over a table of send windows, csrc/grdma_h2_sw.h).  Every link has its device parser, the oracle's parser and its
own SendModel (SH of tests/h2_send_lib.py); the batch helpers of tests/h2_links_send_lib.py run one call over many links
and compare every item exactly with its link's model: result words, windows, counters, progress, slice tables, wire
images.  The cases are small enough for the wave emulator (tests/test_h2_links_send_window_emu.py)."""
import random

import pytest

from oracle import pyorc
from tests.h2_device_lib import FH, SENTINEL, read_slices
from tests.h2_helpers import frame
from tests.h2_links_send_lib import (arrived, by_stream, credit_frames, deframe_all, frame_batch, intake_batch,
                                     intake_batch_raw, model_rounds, place, unfinished)
from tests.h2_send_lib import SH, body, settings, window_update
from tests.h2_send_model import BAD_INCREMENT, LOST, MAXW, STALL_CONN, STALL_STREAM, STALL_UNKNOWN, SendModel

pytestmark = pytest.mark.gpu

PING = frame(6, 0, 0, bytes(8))
COLLIDING = [2 * (3 + 16 * k) + 1 for k in range(8)]   # eight ids of one home slot in a table of 16
WIDE = dict(initial_window=MAXW, conn_window=MAXW, peer_max_frame=(1 << 24) - 1)


def _links(g, n, **kw):
    kw.setdefault("streams", (1, 3))
    kw.setdefault("table_slots", 16)
    return [SH(g, **kw) for _ in range(n)]


def _close(hs):
    for h in hs:
        h.close()


# ---- intake ------------------------------------------------------------------------------------------------------------
CUT_WU = window_update(3, 5) + window_update(1, 0x0a0b0c0d) + window_update(0, 9)
CUT_SETTINGS = settings([(4, 70000), (5, 65536)]) + window_update(1, 3)
SPREAD = window_update(1, 0x01020304) + window_update(0, 7)


def _nine_calls(call):
    """what the nine links receive in the first and in the second call"""
    first = [
        [window_update(0, 1000) + window_update(1, 10) + PING + window_update(3, 20)],   # 0 whole frames
        [SPREAD[k:k + 1] for k in range(len(SPREAD))],                                   # 1 1-byte slices
        [CUT_WU[:13 + 10]], [CUT_WU[:13 + 11]], [CUT_WU[:13 + 12]],                      # 2 3 4 a WINDOW_UPDATE cut
        [CUT_SETTINGS[:9 + 7]],                                                          # 5 a SETTINGS frame cut
        [window_update(1, 5) + window_update(3, 0) + window_update(1, 1 << 31)],         # 6 bad increments
        [settings([(4, 100000)])],                                                       # 7 INITIAL_WINDOW_SIZE, no credit
        [],                                                                              # 8 no events
    ]
    second = [
        [window_update(1, 5)],
        [PING],
        [CUT_WU[13 + 10:]], [CUT_WU[13 + 11:]], [CUT_WU[13 + 12:]],
        [CUT_SETTINGS[9 + 7:]],
        [window_update(0, 0x80000001)],
        [settings([(4, 30)])],
        [],
    ]
    return (first, second)[call]


def test_intake_nine_links_in_shuffled_order_over_two_calls(gpu):
    hs = _links(gpu, 9)
    order = list(range(9))
    random.Random(4).shuffle(order)
    assert order != list(range(9))
    outs = []
    for call in (0, 1):
        deframe_all(hs, _nine_calls(call))
        outs.append(intake_batch(hs, order))
    first, second = outs
    assert first[0] == (3, 1000, 30, 0, 0, 0, 2, 0) and second[0][:3] == (1, 0, 5)
    assert first[1][:3] == (2, 7, 0x01020304) and second[1] == (0, 0, 0, 0, 0, 0, 1, 0)
    for i in (2, 3, 4):   # the carry crosses the batch calls
        assert first[i][:3] == (1, 0, 5) and second[i][:3] == (2, 9, 0x0a0b0c0d), i
        assert hs[i].sw.windows([0, 1, 3]) == [65535 + 9, 65535 + 0x0a0b0c0d, 65540]
    assert first[5][3] == 0 and second[5][3] == 1 and second[5][0] == 1 and hs[5].sw.windows([1]) == [70003]
    assert hs[5].sw.stats()["max_frame"] == 65536
    assert first[6] == (1, 0, 5, 0, BAD_INCREMENT, 3, 1, 0) and second[6][4:6] == (BAD_INCREMENT, 0)
    assert first[7] == (0, 0, 0, 1, 0, 0, 0, 0) and hs[7].sw.windows([1, 3]) == [30, 30]
    assert first[8] == (0, 0, 0, 0, 0, 0, 0, 0) == second[8]
    _close(hs)


def _no_time(st):
    st = dict(st)
    st.pop("kernel_us")
    return st


def test_batch_equals_the_single_calls_on_twin_parsers(gpu):
    from grpc_rdma_amd import h2dev
    batch, single = _links(gpu, 9), _links(gpu, 9)
    for call in (0, 1):
        calls = _nine_calls(call)
        deframe_all(batch, calls)
        deframe_all(single, calls)
        got = h2dev.intake_batch([h.sw for h in batch])
        for i, (hb, h1) in enumerate(zip(batch, single)):
            assert h1.sw.intake() == got[i] == hb.sw.last_result, (call, i)
            assert hb.sw.windows([0, 1, 3]) == h1.sw.windows([0, 1, 3]), (call, i)
            assert _no_time(hb.sw.stats()) == _no_time(h1.sw.stats()), (call, i)
    # the framer: the same tables (one payload arena for both), targets of the same size filled with the sentinel
    kinds = [dict(WIDE), dict(initial_window=1000, conn_window=100), dict(initial_window=40, conn_window=1000)]
    tb = [SH(gpu, streams=(1, 3, 5), table_slots=16, **kw) for kw in kinds]
    t1 = [SH(gpu, streams=(1, 3, 5), table_slots=16, **kw) for kw in kinds]
    msgs = [(body(n, i), (1, 3, 5)[i % 3], i % 4) for i, n in enumerate([0, 700, 0, 9, 1, 30, 200, 4])]
    table = tb[0].upload_bodies(msgs)
    for h in tb + t1:
        h.new_target(256)
    got = h2dev.frame_windowed_batch([(h.sw, table, [0] * len(msgs), 64, h.slices.ptr, 256, h.hdr.ptr, 32 * 256) for h in tb])
    for i, (hb, h1) in enumerate(zip(tb, t1)):
        hb.pay = h1.pay = tb[0].pay
        sl, res, prog = h1.sw.frame(table, [0] * len(msgs), 64, h1.slices.ptr, 256, h1.hdr.ptr, 32 * 256)
        assert got[i][1:] == (res, prog) and res[7] == 0, i
        n = res[2]
        assert place(hb, read_slices(gpu, hb.slices, n)) == place(h1, read_slices(gpu, h1.slices, n)) == place(h1, sl), i
        assert hb.slices.read()[16 * n:] == h1.slices.read()[16 * n:] == bytes([SENTINEL]) * (hb.slices.nbytes - 16 * n)
        assert hb.hdr.read() == h1.hdr.read(), i
        assert hb.sw.windows([0, 1, 3, 5]) == h1.sw.windows([0, 1, 3, 5]), i
        assert _no_time(hb.sw.stats()) == _no_time(h1.sw.stats()), i
    assert got[0][1][0] == len(msgs) and got[1][1][6] == STALL_CONN and got[2][1][6] & STALL_STREAM
    _close(batch + single + tb + t1)


def test_trouble_stays_with_its_link(gpu):
    hs = _links(gpu, 5, streams=(1,))
    cut = window_update(1, 0x0a0b0c0d)
    # 0: a carry, then a call whose event list overflows
    hs[0].feed([window_update(1, 5) + window_update(1, 6)[:11]])
    with pytest.raises(gpu.GrdmaError, match="error 5"):
        hs[0].deframe([window_update(1, 6)[11:]] + [window_update(0, 3)] * 40, ev_cap=16, checked=False)
    # 1: nothing wrong
    hs[1].deframe([window_update(0, 100) + window_update(1, 7)])
    # 2: a connection error
    hs[2].feed([window_update(1, 5)])
    err, _ = hs[2].deframe([window_update(1, 7) + frame(6, 0, 0, b"short") + window_update(1, 9)])
    assert err == 15
    # 3: nothing wrong, with a carry from its last call
    hs[3].feed([cut[:11]])
    hs[3].deframe([cut[11:] + window_update(0, 9)])
    # 4: a standalone deframing that was never taken in
    hs[4].feed([window_update(1, 5) + window_update(1, 0x01000000)[:11]])
    hs[4].deframe([window_update(1, 0x01000000)[11:] + window_update(1, 100)])
    hs[4].model.skipped_call()
    hs[4].deframe([window_update(1, 1)])
    order = [0, 1, 2, 3, 4]
    rc, got = intake_batch_raw(hs, order)
    out = intake_batch(hs, order, lost={0}, got=got)
    assert rc == 4   # (the items whose overflow word is 0)
    assert out[0] == (0, 0, 0, 0, LOST, 0, 1, 2) and hs[0].sw.stats()["lost"]
    assert out[1] == (2, 100, 7, 0, 0, 0, 1, 0) and not hs[1].sw.stats()["lost"]
    assert out[2] == (0, 0, 0, 0, 0, 0, 1, 0) and hs[2].sw.windows([1]) == [65540]
    assert out[3] == (2, 9, 0x0a0b0c0d, 0, 0, 0, 1, 0) and not hs[3].sw.stats()["lost"]
    assert out[4][:3] == (1, 0, 1) and out[4][4] == LOST and hs[4].sw.windows([1]) == [65541]
    # the next call: the lost link starts without its carry, the flag is sticky
    rest = [0, 1, 3, 4]
    deframe_all(hs, [[window_update(1, 2)], [PING], None, [window_update(1, 1)], [window_update(0, 2)]])
    out = intake_batch(hs, rest)
    assert out[0][:3] == (1, 0, 2) and out[0][4] == LOST and out[4][4] == LOST and out[1][4] == 0 == out[3][4]
    _close(hs)


def test_a_share_that_strides(gpu):
    # 2400 frames on eight colliding ids: more than the 2048 threads of a link's share, on two links of one call, with a
    # link that has no events between them
    hs = [SH(gpu, streams=COLLIDING, table_slots=16), SH(gpu, streams=(1,), table_slots=16),
          SH(gpu, streams=COLLIDING, table_slots=16)]
    calls = []
    for seed in (5, 6):
        rng = random.Random(seed)
        frames = [window_update(rng.choice(COLLIDING), rng.randrange(1, 1 << 18)) for _ in range(2400)]
        calls.append([b"".join(frames[k:k + 100]) for k in range(0, 2400, 100)])
    deframe_all(hs, [calls[0], [], calls[1]], ev_cap=8192)
    out = intake_batch(hs, [0, 1, 2])
    assert out[0][0] == 2400 == out[2][0] and out[0][6] == 8 == out[2][6] and out[0][4] == 0 == out[2][4]
    assert out[0][2] != out[2][2] and out[1] == (0, 0, 0, 0, 0, 0, 0, 0)
    _close(hs)


# ---- the framer --------------------------------------------------------------------------------------------------------
def test_framing_links_whose_windows_differ_and_resume(gpu):
    kinds = [
        dict(streams=(1, 3, 5), cap=4096, **WIDE),                                 # 0 open windows
        dict(streams=(1, 3, 5), initial_window=1000, conn_window=100),             # 1 the connection runs out in mid-table
        dict(streams=(1, 3), initial_window=40, conn_window=1000),                 # 2 a stream window binds
        dict(streams=(1,), initial_window=100, conn_window=1000),                  # 3 a negative stream window
        dict(streams=(1,)),                                                        # 4 a stream the map does not hold
        dict(streams=(1, 3, 5), cap=2 * 513 + 8, **WIDE),                          # 5 513 messages: the plan's second block
        dict(streams=(1,)),                                                        # 6 one message
    ]
    hs = [SH(gpu, table_slots=16, **kw) for kw in kinds]
    lens0 = [0, 700, 0, 0, 9, 1, 0, 30, 200, 4]
    msgs = [
        [(body(n, i), (1, 3, 5)[i % 3], (i * 7) % 4) for i, n in enumerate(lens0)],
        [(body(40, 1), 1, 0), (body(40, 2), 3, 0), (body(40, 3), 5, 0), (body(1, 4), 1, 0)],
        [(body(100, 1), 1, 0), (body(20, 2), 3, 0), (body(10, 3), 1, 0), (body(5, 4), 3, 0)],
        [(body(200, 1), 1, 2)],
        [(body(9, 5), 7, 0), (body(20, 1), 1, 0)],
        [(body(i % 7, i), (1, 3, 5)[i % 3], 0) for i in range(513)],
        [(body(50, 1), 1, 2)],
    ]
    mfs = [16384, 16384, 16, 64, 16384, 16384, 16384]
    prog = [[0] * len(m) for m in msgs]
    # link 3: 100 bytes are out, then SETTINGS lowers INITIAL_WINDOW_SIZE below what is in flight
    wire3, _, prog[3] = hs[3].frame(msgs[3], [0], 64)
    hs[3].feed([settings([(4, 30)])])
    assert prog[3] == [100] and hs[3].sw.windows([1]) == [-70]
    exp = frame_batch(hs, list(range(7)), {i: (msgs[i], prog[i], mfs[i]) for i in range(7)})
    res = {i: exp[i][2] for i in exp}
    # open windows: the plain framer's wire
    wire_o, lens_o = pyorc.h2_frame_batch([b for b, _, _ in msgs[0]], [s for _, s, _ in msgs[0]], [f for _, _, f in msgs[0]], 16384)
    assert exp[0][1] == wire_o and exp[0][0] == list(lens_o) and res[0][0] == len(lens0) and res[0][6] == 0
    assert exp[1][3] == [45, 45, 10, 0] and res[1][6] == STALL_CONN and hs[1].sw.windows([0, 1, 3, 5]) == [0, 955, 955, 990]
    assert exp[2][3] == [40, 25, 0, 10] and res[2][6] == STALL_STREAM and hs[2].sw.windows([0, 1, 3]) == [1000 - 75, 0, 5]
    assert exp[3][3] == [100] and res[3][:3] == (0, 1, 0) and exp[3][1] == b"" and res[3][6] == STALL_STREAM
    assert exp[4][3] == [0, 25] and res[4][6] == STALL_UNKNOWN and res[4][:2] == (1, 1)
    assert res[5][:2] == (513, 0) and res[6][:2] == (1, 0) and exp[6][0] == [14, 50]
    # resume: credit through the parsers and intake_batch, frame_windowed_batch again, until every link's messages are out
    out = {i: exp[i][1] for i in exp}
    out[3] = wire3 + out[3]
    hs[4].pp.open([7])
    todo = {}
    for i in range(7):
        t, p = unfinished(msgs[i], exp[i][3])
        if t:
            todo[i] = (t, p)
    assert sorted(todo) == [1, 2, 3, 4]
    rounds = 0
    while todo:
        act = sorted(todo)
        deframe_all(hs, [credit_frames(37, [(s, 61) for s in sorted(hs[i].named)]) if i in todo else None for i in range(7)])
        intake_batch(hs, act)
        exp = frame_batch(hs, act, {i: (todo[i][0], todo[i][1], mfs[i]) for i in act})
        for i in act:
            out[i] += exp[i][1]
            t, p = unfinished(todo[i][0], exp[i][3])
            if t:
                todo[i] = (t, p)
            else:
                del todo[i]
        rounds += 1
        assert rounds < 40
    assert rounds >= 3   # (link 3's window is negative for the first of them)
    for i in range(1, 7):   # (link 0 ends streams in mid-table: its wire is the plain framer's, above)
        assert arrived(out[i], sorted({s for _, s, _ in msgs[i]})) == by_stream(msgs[i]), i
    _close(hs)


def test_emit_across_links(gpu):
    # link 1 has no piece (the connection's window is 0) between two links with pieces; 11 pieces in all: more than the
    # emulator's grid has waves, so the stride wraps; link 0's last piece ends inside the 5-byte message header and leaves
    # an inlined slice of 3 bytes at the back of ITS outbuf, into which a following frame header would merge
    hs = [SH(gpu, streams=(1,), table_slots=16, initial_window=1000, conn_window=4 * 25 + 3),
          SH(gpu, streams=(1,), table_slots=16, conn_window=0),
          SH(gpu, streams=(1, 3), table_slots=16)]
    msgs = [[(body(20, i), 1, 0) for i in range(5)], [(body(20, 7), 1, 0), (body(3, 8), 1, 0)],
            [(body(10, i), (1, 3)[i % 2], 0) for i in range(6)]]
    exp = frame_batch(hs, [0, 1, 2], {i: (msgs[i], [0] * len(msgs[i]), 16384) for i in range(3)})
    assert exp[0][0] == [14, 20] * 4 + [9, 3] and exp[0][3] == [25] * 4 + [3] and exp[0][2][6] == STALL_CONN
    assert exp[1][0] == [] and exp[1][2][:3] == (0, 2, 0) and exp[1][2][5] == 0
    # nothing merged across the boundary: link 2's table begins with its own 14-byte slice at the start of its own arena
    assert exp[2][0] == [14, 10] * 6 and hs[2].last_sl[0] == (hs[2].hdr.ptr, 14)
    assert hs[0].last_sl[-1] == (hs[0].hdr.ptr + 32 * 5, 3)
    # inside link 0 the merge does happen: the next call's first frame header goes on in a fresh outbuf, and a piece
    # that follows a header-only piece in the same call merges (two messages, the first one empty)
    hs[0].feed(credit_frames(1000))
    exp = frame_batch(hs, [2, 0], {0: ([msgs[0][4], (b"", 1, 0), (body(4, 9), 1, 2)], [3, 0, 0], 16384),
                                   2: ([(body(1, 1), 3, 0)], [0], 16384)})
    assert exp[0][0] == [11, 20, 23, 5, 4] and exp[2][0] == [14, 1]
    _close(hs)


def test_a_cap_overflow_in_one_link_only(gpu):
    hs = _links(gpu, 3, initial_window=1000, conn_window=150)
    msgs = [(body(100, 1), 1, 0), (body(100, 2), 3, 0)]
    before = hs[1].sw.windows([0, 1, 3])
    calls = {0: (msgs, [0, 0], 16, 20), 1: (msgs, [0, 0], 16, 5), 2: (msgs, [0, 0], 16, 20)}
    exp = frame_batch(hs, [0, 1, 2], calls)   # (the helper: sentinel kept in link 1's slice table and header arena)
    assert exp[1][2][7] == 1 and exp[1][2][2] == 20 and exp[1][2][5] == 0 and exp[1][3] == [0, 0]
    assert hs[1].sw.windows([0, 1, 3]) == before
    for i in (0, 2):
        assert exp[i][2][7] == 0 and exp[i][3] == [105, 45] and hs[i].sw.windows([0, 1, 3]) == [0, 895, 955]
    # the header cap, and the single call on the same link: -GRDMA_ERR_CAPACITY (SH.frame expects the error)
    exp = frame_batch(hs, [1], {1: (msgs, [0, 0], 16, 20, 32 * 9)})
    assert exp[1][2][7] == 1 and hs[1].sw.windows([0, 1, 3]) == before
    _, res, _ = hs[1].frame(msgs, [0, 0], 16, cap=5)
    assert res[7] == 1
    exp = frame_batch(hs, [1], {1: (msgs, [0, 0], 16, 20)})   # the next call with room is exact
    assert exp[1][2][7] == 0 and exp[1][3] == [105, 45]
    _close(hs)


def test_the_tables_limit(gpu):
    # 256 links of one message each: one link per thread of the emit's prefix scan; every link's connection window
    # differs, so every grant does
    from grpc_rdma_amd import h2dev
    n = 256
    parsers = [h2dev.Parser(False, table_slots=16) for _ in range(n)]
    for p in parsers:
        assert p.open_streams([1]) == 0
    sws = [h2dev.SendWindows(p, 1000, 20 + i, 16384) for i, p in enumerate(parsers)]
    models = [SendModel(1000, 20 + i, 16384) for i in range(n)]
    payload = body(300, 3)
    pay = gpu.DeviceBuffer(data=payload + bytes(16))
    sl = gpu.DeviceBuffer(data=bytes([SENTINEL]) * (64 * n))
    hdr = gpu.DeviceBuffer(data=bytes([SENTINEL]) * (128 * n))
    items = [(sws[i], [(pay.ptr, 300, 1, 2)], [0], 16384, sl.ptr + 64 * i, 4, hdr.ptr + 128 * i, 128) for i in range(n)]
    with pytest.raises(gpu.GrdmaError, match="GRDMA_H2_BATCH_MAX"):
        h2dev.frame_windowed_batch(items + items[:1])
    with pytest.raises(gpu.GrdmaError, match="GRDMA_H2_BATCH_MAX"):
        h2dev.intake_batch(sws + sws[:1])
    got = h2dev.frame_windowed_batch(items)
    tab, arena = sl.read(), hdr.read()
    for i in range(n):
        lens, wire, res, prog = models[i].frame([(payload, 1, 2)], [0], 16384, 4, 128, {1})
        assert got[i][1:] == (res, prog), i
        mine = [(int.from_bytes(tab[o:o + 8], "little"), int.from_bytes(tab[o + 8:o + 16], "little"))
                for o in range(64 * i, 64 * i + 16 * len(lens), 16)]
        assert got[i][0] == mine and [k for _, k in mine] == lens, i
        assert tab[64 * i + 16 * len(lens):64 * i + 64] == bytes([SENTINEL]) * (64 - 16 * len(lens)), i
        out = b""
        for ptr, k in got[i][0]:
            out += arena[ptr - hdr.ptr:ptr - hdr.ptr + k] if hdr.ptr <= ptr < hdr.ptr + 128 * n else payload[ptr - pay.ptr:ptr - pay.ptr + k]
        assert out == wire and res[5] == 20 + i, i
    assert sws[0].windows([0, 1]) == [0, 980] and sws[255].windows([0, 1]) == [0, 1000 - 275]
    for s in sws:
        s.close()
    for p in parsers:
        p.close()


# ---- both halves together ------------------------------------------------------------------------------------------------
def test_round_trip_with_the_ledger_over_two_pairs(gpu):
    # two transport pairs on one device with RFC 7540's default windows: the A sides frame under their windows in one
    # call, the B sides deframe and their ledgers write the WINDOW_UPDATE frames in one call, the A sides deframe those
    # and take them in in one call
    from grpc_rdma_amd import h2dev
    sets = [[(body(200000, 1), 1, 0), (body(200000, 2), 3, 0), (body(200000, 3), 1, 2)],
            [(body(200000, 4), 3, 0), (body(200000, 5), 1, 2), (body(200000, 6), 3, 2)]]
    mfs = [16384, 8192]
    want = [model_rounds(m, mf) for m, mf in zip(sets, mfs)]
    a = [SH(gpu, streams=(1, 3), cap=256, table_slots=16) for _ in range(2)]
    b = [FH(gpu, streams=(1, 3), stream_window=65535, conn_window=65535, conn_threshold=0, max_updates=64, table_slots=16)
         for _ in range(2)]
    todo = {k: (list(sets[k]), [0, 0, 0]) for k in range(2)}
    rounds, got_msgs, partial = [0, 0], [{}, {}], [{}, {}]
    while todo:
        act = sorted(todo)
        exp = frame_batch(a, act, {k: (todo[k][0], todo[k][1], mfs[k]) for k in act})
        for k in act:
            lens, wire, res, prog = exp[k]
            slices, pos = [], 0
            for n in lens:
                slices.append(wire[pos:pos + n])
                pos += n
            b[k].deframe_checked(slices)
            for kind, x, y, c, d, i in b[k].oracle()[1]:
                if kind == pyorc.EV_MSG_BEGIN:
                    partial[k][c] = bytearray()
                elif kind == pyorc.EV_MSG_BYTES:
                    partial[k][c] += slices[i][x:x + y]
                elif kind == pyorc.EV_MSG_END:
                    got_msgs[k].setdefault(c, []).append(bytes(partial[k].pop(c)))
            b[k].new_target()
        back = h2dev.account_batch([(b[k].fc, b[k].slices.ptr, b[k].cap, b[k].hdr.ptr, 32 * b[k].cap) for k in act])
        for j, k in enumerate(act):
            err_o, ev_o = b[k].oracle()
            want_b = b[k].model.call(ev_o, err_o, b[k].cap, 32 * b[k].cap)
            assert want_b[1][5] == 0 and want_b[1][7] == 0
            b[k].check_accounted(want_b, back[j], "ledger %d" % k)
            a[k].deframe([back[j][2]])
        intake_batch(a, act)
        for k in act:
            rounds[k] += 1
            t, p = unfinished(todo[k][0], exp[k][3])
            if t:
                todo[k] = (t, p)
            else:
                del todo[k]
        assert max(rounds) < 100
    assert rounds == want and min(rounds) >= 600000 // 65535
    for k in range(2):
        assert got_msgs[k] == by_stream(sets[k]) and not partial[k]
    _close(a + b)


# ---- refusals and lifetime -------------------------------------------------------------------------------------------------
def _state(h):
    return h.sw.windows([0, 1]), _no_time(h.sw.stats())


def test_refusals_and_lifetime(gpu):
    from grpc_rdma_amd import h2dev
    g = gpu
    x, y = _links(g, 2, streams=(1,))
    t = g.DeviceBuffer(nbytes=8192)
    pay = g.DeviceBuffer(data=body(64))
    ok = [(pay.ptr, 10, 1, 0)]
    good = (y.sw, ok, [0], 16, t.ptr + 4096, 4, t.ptr + 4096 + 256, 128)
    before = [_state(x), _state(y)]

    def refused(call, arg, why):
        with pytest.raises(g.GrdmaError, match=why):
            call(arg)
        assert [_state(x), _state(y)] == before, why

    refused(h2dev.intake_batch, [], "GRDMA_H2_BATCH_MAX")
    refused(h2dev.intake_batch, [x.sw] * 257, "GRDMA_H2_BATCH_MAX")
    refused(h2dev.intake_batch, [x.sw, y.sw], "deframed nothing yet")
    x.deframe([window_update(1, 3)])
    refused(h2dev.intake_batch, [x.sw, y.sw], "deframed nothing yet")   # (y's parser: nothing of x was taken in)
    y.deframe([window_update(0, 4)])
    refused(h2dev.intake_batch, [y.sw, None], "without send windows")
    refused(h2dev.intake_batch, [x.sw, y.sw, x.sw], "twice")
    assert intake_batch([x, y], [0, 1]) == {0: (1, 0, 3, 0, 0, 0, 1, 0), 1: (1, 4, 0, 0, 0, 0, 0, 0)}
    before = [_state(x), _state(y)]
    refused(h2dev.intake_batch, [x.sw, y.sw], "taken in already")
    x.deframe([window_update(1, 5)])
    refused(h2dev.intake_batch, [x.sw, y.sw], "taken in already")       # (y's; x's call is still to be taken in)
    assert intake_batch([x, y], [0])[0][:3] == (1, 0, 5)                 # ... and was not marked taken
    before = [_state(x), _state(y)]
    refused(h2dev.frame_windowed_batch, [], "GRDMA_H2_BATCH_MAX")
    refused(h2dev.frame_windowed_batch, [good] * 257, "GRDMA_H2_BATCH_MAX")
    refused(h2dev.frame_windowed_batch, [good, good], "twice")
    refused(h2dev.frame_windowed_batch, [good, (None,) + good[1:]], "without send windows")
    refused(h2dev.frame_windowed_batch, [good, (x.sw, None, [0], 16, t.ptr, 4, t.ptr + 256, 128)], "message table")
    for msgs, prog, mf, sl, cap, hdr, hdr_cap, why in (
            ([], [], 16, t.ptr, 4, t.ptr + 256, 128, "1 .. 4096"),
            (ok * 4097, [0] * 4097, 16, t.ptr, 4, t.ptr + 256, 128, "1 .. 4096"),
            (ok, [15], 16, t.ptr, 4, t.ptr + 256, 128, "nothing left"),
            ([(pay.ptr, 1 << 32, 1, 0)], [0], 16, t.ptr, 4, t.ptr + 256, 128, "2\\^32"),
            (ok, [0], 0, t.ptr, 4, t.ptr + 256, 128, "max_frame"),
            (ok, [0], 1 << 24, t.ptr, 4, t.ptr + 256, 128, "max_frame"),
            (ok, [0], 16, t.ptr + 8, 4, t.ptr + 256, 128, "misaligned"),
            (ok, [0], 16, 0, 4, t.ptr + 256, 128, "misaligned"),
            (ok, [0], 16, t.ptr, 0, t.ptr + 256, 128, "misaligned"),
            (ok, [0], 16, t.ptr, 4, 0, 128, "misaligned"),
            (ok, [0], 16, t.ptr, 4, t.ptr + 256, 0, "misaligned"),
            (ok, [0], 16, t.ptr, 4, t.ptr + 260, 128, "misaligned")):
        refused(h2dev.frame_windowed_batch, [good, (x.sw, msgs, prog, mf, sl, cap, hdr, hdr_cap)], why)
    # the refusals left both working; after a batch the single calls work on the same objects, and the reverse
    m1, m2 = [(body(30, 1), 1, 0)], [(body(12, 2), 1, 2)]
    exp = frame_batch([x, y], [0, 1], {0: (m1, [0], 16), 1: (m1, [0], 16)})
    assert exp[0][3] == [35] == exp[1][3]
    x.feed([window_update(1, 2)])
    x.frame(m2, [0], 16)
    y.frame(m2, [0], 16)
    deframe_all([x, y], [[window_update(0, 1)], [window_update(1, 8)]])
    intake_batch([x, y], [1, 0])
    exp = frame_batch([x, y], [1, 0], {0: (m2, [0], 5), 1: (m2, [0], 5)})
    assert exp[0][3] == [17] == exp[1][3]
    # a parser destroyed between calls: its send windows refuse, in a batch too; the other link goes on alone
    y.deframe([window_update(1, 1)])
    x.deframe([window_update(1, 1)])
    x.parser.close()
    with pytest.raises(g.GrdmaError, match="parser is gone"):
        h2dev.intake_batch([y.sw, x.sw])
    with pytest.raises(g.GrdmaError, match="parser is gone"):
        h2dev.frame_windowed_batch([good, (x.sw, ok, [0], 16, t.ptr, 4, t.ptr + 256, 128)])
    assert intake_batch([x, y], [1])[1][:3] == (1, 0, 1)
    exp = frame_batch([x, y], [1], {1: (m1, [0], 16)})
    assert exp[1][3] == [35]
    x.sw.close()
    assert x.sw.h is None
    y.close()
