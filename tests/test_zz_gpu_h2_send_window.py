"""Send flow control on the device: the peer's windows and the framer under them (grdma_h2_sw, csrc/grdma_h2_sw.h).
The expected values come from the SendModel of tests/h2_send_model.py: the rules of include/grdma_amd.h applied to the
ORACLE's event list and the bytes fed, the sequential grant, and the oracle's frame_one / sb_add started at an offset.
Every comparison is exact (SH of tests/h2_send_lib.py runs a call on the device and in the model and compares windows,
result blocks, counters, progress, slice lists and wire images)."""
import random

import pytest

from oracle import pyorc
from tests.h2_device_lib import FH, pack_slices, same
from tests.h2_flow_model import Model as LedgerModel
from tests.h2_helpers import frame, grpc_msg, grpcio_capture
from tests.h2_send_lib import SH, body, settings, window_update
from tests.h2_send_model import (BAD_INCREMENT, BAD_SETTINGS, LOST, MAXW, STALL_CONN, STALL_STREAM, STALL_UNKNOWN,
                                 WINDOW_OVERFLOW, SendModel)

pytestmark = pytest.mark.gpu

PING = frame(6, 0, 0, bytes(8))


# ---- intake --------------------------------------------------------------------------------------------------------------
def test_window_updates_whole_in_one_slice(gpu):
    h = SH(gpu, streams=(1, 3, 5))
    res = h.feed([window_update(0, 1000) + window_update(1, 10) + PING + window_update(3, 20) + window_update(5, 30)])
    assert res == (4, 1000, 60, 0, 0, 0, 3, 0)
    assert h.sw.windows([0, 1, 3, 5, 7]) == [66535, 65545, 65555, 65565, 65535]
    res = h.feed([PING])  # (a call without control frames)
    assert res == (0, 0, 0, 0, 0, 0, 3, 0)
    h.close()


@pytest.mark.parametrize("cuts", [(10,), (11,), (12,), (10, 12), (9, 11), (10, 11, 12), (3, 9, 10, 13)])
def test_increment_spread_over_slices(gpu, cuts):
    h = SH(gpu, streams=(1,))
    w = window_update(1, 0x01020304) + window_update(0, 7)
    cuts = (0,) + cuts + (len(w),)
    res = h.feed([w[a:b] for a, b in zip(cuts, cuts[1:])])
    assert res[:3] == (2, 7, 0x01020304)
    h.close()


@pytest.mark.parametrize("cut", [4, 9, 10, 11, 12])
def test_call_cut_inside_a_window_update(gpu, cut):
    # inside the 9-byte header, and after 0, 1, 2 and 3 payload bytes: the carry
    h = SH(gpu, streams=(1, 3))
    w = window_update(3, 5) + window_update(1, 0x0a0b0c0d) + window_update(0, 9)
    at = 13 + cut
    res = h.feed([w[:at]])
    assert res[:3] == (1, 0, 5)
    res = h.feed([w[at:]])
    assert res[:3] == (2, 9, 0x0a0b0c0d) and h.sw.windows([1]) == [65535 + 0x0a0b0c0d]
    # a frame cut twice: a call that delivers one byte of it
    w = window_update(1, 0x00010203)
    h.feed([w[:10]])
    assert h.feed([w[10:11]])[0] == 0
    assert h.feed([w[11:]])[:3] == (1, 0, 0x00010203)
    h.close()


def test_settings(gpu):
    h = SH(gpu, streams=(1,))
    # both ids and unknown ones; an entry given twice: the later one holds
    res = h.feed([settings([(1, 4096), (4, 100000), (3, 100), (5, 32768), (4, 200000), (0xfff0, 1)])])
    assert res == (0, 0, 0, 1, 0, 0, 0, 0)
    st = h.sw.stats()
    assert (st["initial_window"], st["max_frame"]) == (200000, 32768) and h.sw.windows([1, 9]) == [200000, 200000]
    # two frames in one call: the last wins, value by value; an ACK and an empty frame change nothing
    res = h.feed([settings([(4, 300000), (5, 20000)]) + settings([], ack=True) + settings([(4, 400000)]), settings([])])
    assert res[3] == 3
    st = h.sw.stats()
    assert (st["initial_window"], st["max_frame"]) == (400000, 20000)
    h.close()


@pytest.mark.parametrize("cut", range(13))
def test_settings_cut_between_calls(gpu, cut):
    # a 12-byte payload cut at each of its 13 positions: nothing applies before the last byte
    h = SH(gpu, streams=(1,))
    s = settings([(4, 70000), (5, 65536)]) + window_update(1, 3)
    at = 9 + cut
    res = h.feed([s[:at]])
    st = h.sw.stats()
    assert res[3] == (1 if cut == 12 else 0) and st["initial_window"] == (70000 if cut == 12 else 65535)
    res = h.feed([s[at:]])
    st = h.sw.stats()
    assert res[3] == (0 if cut == 12 else 1) and (st["initial_window"], st["max_frame"]) == (70000, 65536)
    assert h.sw.windows([1]) == [70003]
    h.close()


def test_violations(gpu):
    h = SH(gpu, streams=(1, 3))
    res = h.feed([window_update(1, 5) + window_update(3, 0) + window_update(1, 1 << 31) + window_update(0, 0)])
    assert res == (1, 0, 5, 0, BAD_INCREMENT, 3, 1, 0) and h.sw.stats()["violations"] == 3
    res = h.feed([PING + window_update(0, 0x80000001)])
    assert res[4] == BAD_INCREMENT and res[5] == 0
    res = h.feed([window_update(1, 1) + settings([(4, 1 << 31), (5, 16383), (5, 1 << 24), (5, 16384)])])
    st = h.sw.stats()
    assert res[3:6] == (1, BAD_SETTINGS, 0) and (st["initial_window"], st["max_frame"], st["violations"]) == (65535, 16384, 7)
    # windows pushed past 2^31 - 1 stay there
    res = h.feed([window_update(3, MAXW - 65535) + window_update(3, 1)])
    assert res == (2, 0, MAXW - 65535, 0, WINDOW_OVERFLOW, 3, 2, 0) and h.sw.windows([3]) == [MAXW]
    res = h.feed([window_update(0, MAXW) + window_update(1, 2)])
    assert res == (2, MAXW - 65535, 2, 0, WINDOW_OVERFLOW, 0, 2, 0) and h.sw.windows([0, 1]) == [MAXW, 65535 + 8]
    # a lowered INITIAL_WINDOW_SIZE makes room again: the clamp is judged with the call's own SETTINGS
    res = h.feed([window_update(3, 10) + settings([(4, 65535 - 100)])])
    assert res[4] == 0 and h.sw.windows([3]) == [MAXW - 90]
    h.close()


def test_calls_that_cannot_be_taken_in(gpu):
    h = SH(gpu, streams=(1,))
    h.feed([window_update(1, 5)])
    # a connection error: nothing is taken in
    err, _ = h.deframe([window_update(1, 7) + frame(6, 0, 0, b"short") + window_update(1, 9)])
    assert err == 15
    assert h.intake() == (0, 0, 0, 0, 0, 0, 1, 0) and h.sw.windows([1]) == [65540]
    h.close()
    # an event overflow: the sticky flag, -GRDMA_ERR_CAPACITY, nothing else
    h = SH(gpu, streams=(1,))
    h.feed([window_update(1, 5) + window_update(1, 6)[:11]])
    with pytest.raises(gpu.GrdmaError, match="error 5"):
        h.deframe([window_update(1, 6)[11:]] + [window_update(0, 3)] * 40, ev_cap=16, checked=False)
    with pytest.raises(gpu.GrdmaError, match="error 5"):
        h.sw.intake()
    same(h.sw.last_result, h.model.lost_call(), "the lost call's result")
    assert h.sw.last_result == (0, 0, 0, 0, LOST, 0, 1, 2)
    h.check()
    with pytest.raises(gpu.GrdmaError, match="taken in already"):
        h.sw.intake()
    h.close()
    # a standalone deframing that was never taken in: the flag in every later result block, the windows keep what they know
    h = SH(gpu, streams=(1,))
    h.feed([window_update(1, 5) + window_update(1, 0x01000000)[:11]])
    h.deframe([window_update(1, 0x01000000)[11:] + window_update(1, 100)])  # (never taken in)
    h.model.skipped_call()
    res = h.feed([window_update(1, 1)])
    assert res[:3] == (1, 0, 1) and res[4] == LOST and h.sw.windows([1]) == [65541]
    res = h.feed([window_update(0, 2)])
    assert res[:2] == (1, 2) and res[4] == LOST and h.sw.stats()["lost"]
    h.close()


def test_colliding_streams_under_many_frames(gpu):
    # 2400 frames on eight ids of one home slot in a table of 16: sums exact (on the device the frames of one stream are
    # added by many workgroups at once)
    ids = [2 * (3 + 16 * k) + 1 for k in range(8)]
    h = SH(gpu, streams=ids, table_slots=16)
    rng = random.Random(5)
    frames = [window_update(rng.choice(ids), rng.randrange(1, 1 << 18)) for _ in range(2400)]
    res = h.feed([b"".join(frames[k:k + 100]) for k in range(0, 2400, 100)], ev_cap=8192)
    assert res[0] == 2400 and res[6] == 8 and res[4] == 0
    h.close()


def test_the_table_follows_the_stream_map(gpu):
    # clusters around the table's end: homes 14, 15, 0, 1 of 16 slots, two ids on 14
    ids = [29, 61, 31, 33, 35]
    h = SH(gpu, streams=ids, table_slots=16)
    h.named.add(7)
    res = h.feed([b"".join(window_update(s, 10 + s) for s in ids) + window_update(7, 99)])  # (7: unknown, ignored)
    assert res[0] == 5 and res[6] == 5 and h.sw.windows([7]) == [65535]
    # RST_STREAM takes 61 out of the map; 31 ends its reads, then the host closes its writes
    res = h.feed([frame(3, 0, 61, bytes(4)) + window_update(61, 5) + frame(0, 1, 31, grpc_msg(b"x"))])
    assert res[0] == 0 and res[6] == 4 and h.sw.windows([61, 31]) == [65535, 65535 + 41]
    h.pp.close_writes([31])
    res = h.feed([window_update(29, 1)])
    assert res[6] == 3 and h.sw.windows([29, 31, 33, 35]) == [65535 + 40, 65535, 65535 + 43, 65535 + 45]
    # the same id opened again starts fresh
    h.pp.open([61])
    res = h.feed([window_update(61, 2)])
    assert res[6] == 4 and h.sw.windows([61]) == [65537]
    h.close()


@pytest.mark.parametrize("seed", [None, 1, 2])
def test_grpcio_capture(gpu, seed):
    data, _ = grpcio_capture()
    h = SH(gpu, prefix=True)
    h.named |= {1, 3, 5, 7, 9}
    if seed is None:
        calls = [[data]]
    else:
        rng = random.Random(seed)
        cuts = sorted(rng.sample(range(1, len(data)), 12))
        pieces = [data[a:b] for a, b in zip([0] + cuts, cuts + [len(data)])]
        calls = [pieces[k:k + 3] for k in range(0, len(pieces), 3)]
    total = [0, 0, 0]
    for slices in calls:
        res = h.feed(slices)
        assert res[4] == 0 and res[7] == 0
        total = [total[0] + res[0], total[1] + res[1], total[2] + res[3]]
    st = h.sw.stats()
    assert (st["initial_window"], st["max_frame"]) == (4194304, 4194304) and total[2] == 1
    assert h.sw.windows([0]) == [65535 + 4128769 + 5] and total[1] == 4128769 + 5
    assert total[0] >= 2  # (the stream frames count where the map still holds their stream at the call's end)
    h.close()


# ---- the framer ----------------------------------------------------------------------------------------------------------
def _open(gpu, streams=(1, 3, 5), **kw):
    return SH(gpu, streams=streams, initial_window=MAXW, conn_window=MAXW, peer_max_frame=(1 << 24) - 1, **kw)


@pytest.mark.parametrize("mf", [1, 5, 6, 16384])
def test_open_windows_equal_the_plain_framer(gpu, mf):
    from grpc_rdma_amd import h2dev
    lens = [0, 700, 0, 0, 9, 1, 0, 30, 200, 4] if mf > 1 else [0, 9, 0, 0, 1, 30]
    msgs = [(body(n, i), (1, 3, 5)[i % 3], (i * 7) % 4) for i, n in enumerate(lens)]
    h = _open(gpu, cap=4096)
    wire, res, prog = h.frame(msgs, [0] * len(msgs), mf)
    assert res[0] == len(msgs) and res[6] == 0 and prog == [5 + n for n in lens]
    wire_o, lens_o = pyorc.h2_frame_batch([b for b, _, _ in msgs], [s for _, s, _ in msgs], [f for _, _, f in msgs], mf)
    assert wire == wire_o and res[2] == len(lens_o)
    # grdma_h2_frame_messages on the same table
    table = h.upload_bodies(msgs)
    sl = gpu.DeviceBuffer(nbytes=16 * 4096)
    hdr = gpu.DeviceBuffer(nbytes=32 * 4096)
    n, wire_bytes = h2dev.frame_messages(table, mf, sl.ptr, 4096, hdr.ptr, 32 * 4096)
    assert (n, wire_bytes) == (res[2], res[4])
    raw = sl.read(16 * n)
    assert [int.from_bytes(raw[16 * i + 8:16 * i + 16], "little") for i in range(n)] == lens_o
    h.close()


def _credit(h, conn=0, streams=()):
    """real WINDOW_UPDATE bytes through the parser and the intake"""
    frames = ([window_update(0, conn)] if conn else []) + [window_update(s, n) for s, n in streams if n]
    if frames:
        h.feed([b"".join(frames)])


def _drain(h, msgs, mf, credit, prog=None, out=b"", limit=200):
    """give credit, frame, and again until everything is out -> (the concatenated wire behind `out`, calls)"""
    prog = prog if prog is not None else [0] * len(msgs)
    keep = [i for i, (b, _, _) in enumerate(msgs) if prog[i] < 5 + len(b)]
    todo, prog, calls = [msgs[i] for i in keep], [prog[i] for i in keep], 0
    while todo:
        credit(h)
        wire, res, prog = h.frame(todo, prog, mf)
        out += wire
        keep = [i for i, (b, _, _) in enumerate(todo) if prog[i] < 5 + len(b)]
        todo, prog = [todo[i] for i in keep], [prog[i] for i in keep]
        calls += 1
        assert calls < limit
    return out, calls


def _arrived(wire, streams):
    """the wire through the oracle's parser -> {stream: [message, ...]}"""
    orc = pyorc.H2Parser(False)
    for s in streams:
        assert orc.open_stream(s) == 0
    rc, ev = orc.feed(wire)
    assert rc == 0
    back, partial = {}, {}
    for k, a, b, c, d in ev:
        if k == pyorc.EV_MSG_BEGIN:
            partial[c] = bytearray()
        elif k == pyorc.EV_MSG_BYTES:
            partial[c] += wire[a:a + b]
        elif k == pyorc.EV_MSG_END:
            back.setdefault(c, []).append(bytes(partial.pop(c)))
    assert not partial
    return back


def _by_stream(msgs):
    want = {}
    for b, s, _ in msgs:
        want.setdefault(s, []).append(b)
    return want


@pytest.mark.parametrize("window", list(range(15)) + [19, 20, 21])
def test_connection_window_edges(gpu, window):
    # cuts at each byte of the 5-byte header and just behind it, and around a frame's end (mf = 20)
    h = SH(gpu, streams=(1, 3), conn_window=window)
    msgs = [(body(30, 1), 1, 0), (b"", 3, 0), (body(50, 2), 3, 2)]
    wire, res, prog = h.frame(msgs, [0, 0, 0], 20)
    assert res[5] == min(window, 35 + 5 + 55) == sum(prog) and res[6] == STALL_CONN
    out, _ = _drain(h, msgs, 20, lambda hh: _credit(hh, conn=7), prog, wire)
    assert _arrived(out, (1, 3)) == _by_stream(msgs)
    h.close()


def test_stream_windows(gpu):
    # a stream window below the connection's; two streams interleaved, one stalled, the other running; a second message
    # held behind its unfinished first; an unknown stream
    h = SH(gpu, streams=(1, 3), initial_window=40, conn_window=1000)
    msgs = [(body(100, 1), 1, 0), (body(20, 2), 3, 0), (body(10, 3), 1, 0), (body(5, 4), 3, 0), (body(9, 5), 7, 0)]
    wire, res, prog = h.frame(msgs, [0] * 5, 16)
    assert prog == [40, 25, 0, 10, 0] and res[:2] == (2, 3) and res[6] == STALL_STREAM | STALL_UNKNOWN
    assert h.sw.windows([0, 1, 3, 7]) == [1000 - 75, 0, 5, 40]
    # stream 1 gets credit for less than its first message: the second stays held
    _credit(h, streams=[(1, 50)])
    wire, res, prog = h.frame([msgs[0], msgs[2]], [40, 0], 16)
    assert prog == [90, 0] and res[6] == STALL_STREAM
    _credit(h, streams=[(1, 20)])
    wire, res, prog = h.frame([msgs[0], msgs[2]], [90, 0], 16)
    assert prog == [105, 5] and res[:2] == (1, 1)
    h.close()


def test_connection_window_runs_out_in_mid_table(gpu):
    h = SH(gpu, streams=(1, 3, 5), initial_window=1000, conn_window=100)
    msgs = [(body(40, 1), 1, 0), (body(40, 2), 3, 0), (body(40, 3), 5, 0), (body(1, 4), 1, 0)]
    wire, res, prog = h.frame(msgs, [0] * 4, 16384)
    assert prog == [45, 45, 10, 0] and res[6] == STALL_CONN and h.sw.windows([0, 1, 3, 5]) == [0, 955, 955, 990]
    out, _ = _drain(h, msgs, 16384, lambda hh: _credit(hh, conn=11), prog, wire)
    assert _arrived(out, (1, 3, 5)) == _by_stream(msgs)
    h.close()


def test_negative_stream_window(gpu):
    # SETTINGS lowers INITIAL_WINDOW_SIZE below what is in flight; a WINDOW_UPDATE lifts the window again
    h = SH(gpu, streams=(1,), initial_window=100, conn_window=1000)
    msgs = [(body(200, 1), 1, 2)]
    wire, res, prog = h.frame(msgs, [0], 64)
    assert prog == [100]
    h.feed([settings([(4, 30)])])
    assert h.sw.windows([1]) == [-70]
    wire, res, prog = h.frame(msgs, [100], 64)
    assert prog == [100] and res[:2] == (0, 1) and res[2] == 0 and wire == b"" and res[6] == STALL_STREAM
    _credit(h, streams=[(1, 60)])
    wire, res, prog = h.frame(msgs, [100], 64)
    assert prog == [100] and h.sw.windows([1]) == [-10]
    _credit(h, streams=[(1, 200)])
    wire, res, prog = h.frame(msgs, [100], 64)
    assert prog == [205] and res[:2] == (1, 0) and wire[4] == 0 and wire[9 + 64 + 4] == 1  # (END_STREAM on the last frame only)
    h.close()


@pytest.mark.parametrize("seed", range(6))
def test_resume_until_everything_is_out(gpu, seed):
    rng = random.Random(100 + seed)
    lens = [rng.choice((0, 1, 4, 9, 30, 200, 700)) for _ in range(rng.randrange(3, 10))]
    msgs = [(body(n, i), rng.choice((1, 3, 5)), rng.randrange(2)) for i, n in enumerate(lens)]
    mf = rng.choice((1, 5, 6, 7, 23, 100)) if max(lens) < 200 else rng.choice((6, 7, 23, 100))
    h = SH(gpu, streams=(1, 3, 5), initial_window=rng.randrange(0, 30), conn_window=rng.randrange(0, 30), cap=2048)

    def credit(hh):
        _credit(hh, conn=rng.randrange(0, 300), streams=[(s, rng.randrange(0, 200)) for s in (1, 3, 5)])
    out, calls = _drain(h, msgs, mf, credit)
    assert _arrived(out, (1, 3, 5)) == _by_stream(msgs) and calls >= 1
    h.close()


def test_many_messages_on_one_stream(gpu):
    # 4096 messages of one stream, the stream's window ends inside message 3000
    n = 4096
    msgs = [(body(100, i), 1, 0) for i in range(n)]
    h = SH(gpu, streams=(1,), initial_window=3000 * 105 + 50, conn_window=MAXW, cap=2 * n + 8)
    wire, res, prog = h.frame(msgs, [0] * n, 16384)
    assert res[:2] == (3000, n - 3000) and prog[2999:3002] == [105, 50, 0] and res[6] == STALL_STREAM
    _credit(h, streams=[(1, 1 << 20)])
    wire, res, prog = h.frame(msgs[3000:], prog[3000:], 16384)
    assert res[:2] == (n - 3000, 0) and res[6] == 0
    h.close()


def test_many_streams(gpu):
    # 2048 streams x 2 messages; every stream's window ends inside its second message, the connection's in the second half
    ids = [2 * k + 1 for k in range(2048)]
    msgs = [(body(100, s), s, 0) for s in ids] + [(body(100, s + 1), s, 2) for s in ids]
    h = SH(gpu, streams=ids, table_slots=4096, initial_window=150, conn_window=2048 * 105 + 1000 * 45 + 20, cap=2 * 4096 + 8)
    wire, res, prog = h.frame(msgs, [0] * 4096, 1 << 20)
    assert res[:2] == (2048, 2048) and res[6] == STALL_CONN | STALL_STREAM
    assert prog[2048:2048 + 1002] == [45] * 1000 + [20, 0] and h.sw.windows([0, 1, 2001, 2003]) == [0, 0, 25, 45]
    h.close()


def test_a_cap_overflow_writes_nothing(gpu):
    h = SH(gpu, streams=(1, 3), initial_window=1000, conn_window=150)
    msgs = [(body(100, 1), 1, 0), (body(100, 2), 3, 0)]
    before = h.sw.windows([0, 1, 3])
    wire, res, prog = h.frame(msgs, [0, 0], 16, cap=5)           # the slice cap
    assert res[7] == 1 and res[2] == 20 and prog == [0, 0] and h.sw.windows([0, 1, 3]) == before
    wire, res, prog = h.frame(msgs, [0, 0], 16, cap=20, hdr_cap=32 * 9)  # the header cap
    assert res[7] == 1 and h.sw.windows([0, 1, 3]) == before
    wire, res, prog = h.frame(msgs, [0, 0], 16, cap=20)          # the next call with room is exact
    assert res[7] == 0 and prog == [105, 45] and h.sw.windows([0, 1, 3]) == [0, 895, 955]
    h.close()


def test_refusals_and_lifetime(gpu):
    g = gpu
    from grpc_rdma_amd import h2dev
    parser = h2dev.Parser(False)
    assert parser.open_streams([1]) == 0
    for kw in (dict(initial_window=1 << 31), dict(conn_window=1 << 31), dict(peer_max_frame=16383), dict(peer_max_frame=1 << 24)):
        with pytest.raises(g.GrdmaError):
            h2dev.SendWindows(parser, **kw)
    sw = h2dev.SendWindows(parser)
    with pytest.raises(g.GrdmaError, match="send windows already"):
        h2dev.SendWindows(parser)
    with pytest.raises(g.GrdmaError, match="deframed nothing yet"):
        sw.intake()
    data, table = pack_slices([window_update(1, 3)])
    buf = g.DeviceBuffer(data=data)
    parser.deframe(buf.ptr, table)
    assert sw.intake()[:3] == (1, 0, 3)
    with pytest.raises(g.GrdmaError, match="taken in already"):
        sw.intake()
    t = g.DeviceBuffer(nbytes=4096)
    pay = g.DeviceBuffer(data=body(64))
    ok = [(pay.ptr, 10, 1, 0)]
    for msgs, prog, mf, sl, cap, hdr, hdr_cap, why in (
            ([], [], 16, t.ptr, 4, t.ptr + 256, 128, "1 .. 4096"),
            (ok * 4097, [0] * 4097, 16, t.ptr, 4, t.ptr + 256, 128, "1 .. 4096"),
            (ok, [15], 16, t.ptr, 4, t.ptr + 256, 128, "nothing left"),
            (ok, [0], 0, t.ptr, 4, t.ptr + 256, 128, "max_frame"),
            (ok, [0], 1 << 24, t.ptr, 4, t.ptr + 256, 128, "max_frame"),
            (ok, [0], 16, t.ptr + 8, 4, t.ptr + 256, 128, "misaligned"),
            (ok, [0], 16, t.ptr, 0, t.ptr + 256, 128, "misaligned"),
            (ok, [0], 16, t.ptr, 4, 0, 128, "misaligned"),
            (ok, [0], 16, t.ptr, 4, t.ptr + 260, 128, "misaligned")):
        with pytest.raises(g.GrdmaError, match=why):
            sw.frame(msgs, prog, mf, sl, cap, hdr, hdr_cap)
    sl, res, prog = sw.frame(ok, [0], 16, t.ptr, 4, t.ptr + 256, 128)  # (the refusals left it working)
    assert prog == [15] and res[:2] == (1, 0)
    sw.close()
    assert sw.h is None
    sw = h2dev.SendWindows(parser)  # (the parser is free again; the deframing in front of it is not its business)
    with pytest.raises(g.GrdmaError, match="taken in already"):
        sw.intake()
    # a parser closed before its send windows: they refuse every call and can still be closed
    parser.close()
    with pytest.raises(g.GrdmaError, match="parser is gone"):
        sw.intake()
    with pytest.raises(g.GrdmaError, match="parser is gone"):
        sw.frame(ok, [0], 16, t.ptr, 4, t.ptr + 256, 128)
    sw.close()
    assert sw.h is None


# ---- both halves together ---------------------------------------------------------------------------------------------
def _model_rounds(msgs, mf):
    """side A's SendModel against side B's ledger model, both fed by the oracle's parsers -> rounds until done"""
    a, b = SendModel(), LedgerModel(65535, 65535, 0, 64, (1, 3))
    orc_a, orc_b = pyorc.H2Parser(False), pyorc.H2Parser(False)
    for s in (1, 3):
        assert orc_a.open_stream(s) == 0 and orc_b.open_stream(s) == 0
    todo, prog, rounds = list(msgs), [0] * len(msgs), 0
    while todo:
        lens, wire, res, prog = a.frame(todo, prog, mf, 1 << 20, 1 << 30, {1, 3})
        keep = [i for i, (m, _, _) in enumerate(todo) if prog[i] < 5 + len(m)]
        todo, prog = [todo[i] for i in keep], [prog[i] for i in keep]
        rc, ev = orc_b.feed(wire, cap=len(wire) + 4096)
        assert rc == 0
        _, res_b, back = b.call(ev, 0, 64, 32 * 64)
        assert res_b[5] == 0
        rc, ev = orc_a.feed(back)
        assert rc == 0
        a.intake([e + (0,) for e in ev], [back], 0, {1, 3})
        rounds += 1
        assert rounds < 100
    return rounds


def test_round_trip_with_the_ledger(gpu):
    # two transports on one device with RFC 7540's default windows: A frames under its windows, B deframes and its
    # ledger writes the WINDOW_UPDATE frames, A deframes those and takes them in
    msgs = [(body(200000, 1), 1, 0), (body(200000, 2), 3, 0), (body(200000, 3), 1, 2)]
    want_rounds = _model_rounds(msgs, 16384)
    a = SH(gpu, streams=(1, 3), cap=256)
    b = FH(gpu, streams=(1, 3), stream_window=65535, conn_window=65535, conn_threshold=0, max_updates=64)
    todo, prog, rounds, arrived, partial = list(msgs), [0] * len(msgs), 0, {}, {}
    while todo:
        a.frame(todo, prog, 16384)
        lens, wire, res, prog = a.last_frame
        keep = [i for i, (m, _, _) in enumerate(todo) if prog[i] < 5 + len(m)]
        todo, prog = [todo[i] for i in keep], [prog[i] for i in keep]
        slices, pos = [], 0
        for n in lens:
            slices.append(wire[pos:pos + n])
            pos += n
        res_b, back = b.feed(slices)
        assert res_b[5] == 0 and res_b[7] == 0
        for k, x, y, c, d, i in b.oracle()[1]:
            if k == pyorc.EV_MSG_BEGIN:
                partial[c] = bytearray()
            elif k == pyorc.EV_MSG_BYTES:
                partial[c] += slices[i][x:x + y]
            elif k == pyorc.EV_MSG_END:
                arrived.setdefault(c, []).append(bytes(partial.pop(c)))
        a.feed([back])
        rounds += 1
        assert rounds < 100
    assert arrived == _by_stream(msgs) and not partial
    assert rounds == want_rounds and rounds >= 600000 // 65535
    a.close()
    b.close()
