"""Replies under the peer's windows: grdma_h2_reply_attach_windows / grdma_h2_reply_frame_windowed (k_h2_wr_queue,
k_h2_sw_plan, k_h2_sw_emit, k_h2_wr_commit; csrc/grdma_h2_wr.h).  The expected values come from
tests/h2_windowed_reply_model.py, which tests/test_h2_windowed_reply_model.py pins against the oracle; WH of
tests/h2_windowed_reply_lib.py runs every call on the device and in the model and compares exactly: slice list, whole
slice table and header arena, result block, windows, the queue's progress, the assembler's bytes in use."""
import pytest

from tests.h2_device_lib import FH, RHarness, Target, _dropped_slices, expected_reply, same
from tests.h2_helpers import frame, grpc_msg
from tests.h2_send_lib import body, settings, window_update
from tests.h2_send_model import MAXW, STALL_CONN, STALL_STREAM
from tests.h2_windowed_reply_lib import WH, Peer, data, drain, rst

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("mf", [16384, 6, 1])
def test_open_windows_equal_reply_frame_on_a_twin(gpu, mf):
    from grpc_rdma_amd import h2dev
    lens = [0, 700, 0, 0, 9, 1, 0, 30, 200, 4] if mf > 1 else [0, 9, 0, 0, 1, 30]
    slices = [f for i, n in enumerate(lens) for f in data((1, 3, 5)[i % 3], body(n, i), i & 1)]
    h = WH(gpu, initial_window=MAXW, conn_window=MAXW, peer_max_frame=(1 << 24) - 1, max_frame=mf, cap=4096)
    h.receive(slices)
    wire, res = h.frame()
    assert res[:2] == (len(lens), 0) and res[5] == sum(5 + n for n in lens) and res[6:8] == (0, 0) and res[12] == len(lens)
    exp = expected_reply(h.r.last, mf)
    assert (wire, len(h.last_slices)) == (exp[0], len(exp[1]))
    # grdma_h2_reply_frame over the same call of a twin: the same slice list, pointer for pointer
    t = RHarness(gpu, 1 << 16, streams=(1, 3, 5))
    t.feed(slices)
    plain = h2dev.Reply(t.asm, None, mf)
    tg = Target(gpu, 4096)
    n, st = tg.frame(plain)
    _, wire_t, got = tg.wire(n)

    def rel(sl, hdr, arena):
        return [("h", p - hdr.ptr, k) if hdr.ptr <= p < hdr.ptr + hdr.nbytes else ("a", p - arena.ptr, k) for p, k in sl]
    assert wire_t == wire and rel(got, tg.hdr, t.arena) == rel(h.last_slices, h.hdr, h.r.arena)
    assert (st["slices"], st["hdr_bytes"], st["wire_bytes"]) == res[2:5]
    assert h.hdr.read(st["hdr_bytes"]) == tg.hdr.read(st["hdr_bytes"])
    plain.close()
    t.close()
    h.close()


def test_a_message_against_its_stream_window_then_the_rest(gpu):
    h = WH(gpu, initial_window=100, conn_window=65535)
    peer = Peer((1, 3, 5))
    h.receive(data(1, body(200, 1)))
    wire, res = h.frame()
    peer.feed(wire)
    assert res[:2] == (0, 1) and res[5] == 100 and res[6] == STALL_STREAM and res[8] == 1 and res[12] == 0
    assert h.reply.pending() == [(1, 200, 100)]
    h.credit([window_update(1, 500)])
    wire, res = h.frame()  # (the source call is taken already: the queue alone)
    peer.feed(wire)
    assert res[:2] == (1, 0) and res[5] == 105 and res[8] == 0 and res[12] == 1 and h.reply.pending() == []
    assert peer.got == {1: [body(200, 1)]} and not peer.partial
    h.release()
    assert h.r.asm.stats()["bytes_in_use"] == 0
    h.close()


@pytest.mark.parametrize("window", [0, 3, 5, 6])
def test_small_stream_windows(gpu, window):
    # cuts inside the 5-byte header, just behind it and one byte into the payload; an empty message behind the cut one
    h = WH(gpu, initial_window=window, conn_window=1000, max_frame=20)
    peer = Peer((1, 3, 5))
    h.receive(data(1, body(30, 1)) + data(1, b"") + data(3, b"") + data(3, body(50, 2), 1))
    wire, res = h.frame()
    peer.feed(wire)
    assert res[5] == 2 * min(window, 5 + 30) if window < 5 else res[5] == min(window, 35) + 5 + min(window - 5, 55)
    drain(h, peer, [window_update(1, 7) + window_update(3, 9)])
    assert peer.got == {1: [body(30, 1), b""], 3: [b"", body(50, 2)]} and not peer.partial
    h.close()


def test_connection_window_across_streams_and_old_entries_in_front(gpu):
    h = WH(gpu, initial_window=50, conn_window=120)
    peer = Peer((1, 3, 5))
    h.receive(data(1, body(100, 1)) + data(3, body(40, 2)) + data(5, body(40, 3)) + data(1, body(5, 4)))
    wire, res = h.frame()
    peer.feed(wire)
    # stream 1 is cut by its window, so its later message gets nothing; the connection's window ends inside stream 5's
    assert h.reply.pending() == [(1, 100, 50), (5, 40, 25), (1, 5, 0)] and res[:2] == (1, 3)
    assert res[6] == STALL_CONN | STALL_STREAM and res[12] == 0
    # what waited goes in front of what arrives: per-stream order is the queue's order
    h.receive(data(5, body(7, 5)) + data(3, body(8, 6)) + data(1, body(9, 7)))
    h.credit([window_update(0, 60) + window_update(1, 30)])
    wire, res = h.frame()
    peer.feed(wire)
    assert res[8] == 3 and h.reply.pending() == [(1, 100, 80), (1, 5, 0), (5, 7, 5), (3, 8, 5), (1, 9, 0)]
    assert res[:2] == (1, 5) and res[12] == 0  # (stream 1's first message, the oldest of all, still pins the ring)
    drain(h, peer, [window_update(0, 500) + b"".join(window_update(s, 500) for s in (1, 3, 5))])
    assert peer.got == {1: [body(100, 1), body(5, 4), body(9, 7)], 3: [body(40, 2), body(8, 6)], 5: [body(40, 3), body(7, 5)]}
    h.release()
    assert h.r.asm.stats()["bytes_in_use"] == 0
    h.close()


def test_inlined_run_across_the_old_new_boundary(gpu):
    # an empty message cut inside its header waits; behind it empty messages arrive: one run of inlined slices
    h = WH(gpu, initial_window=3, conn_window=1000)
    peer = Peer((1, 3, 5))
    h.receive(data(1, b"") + data(3, b""))
    wire, res = h.frame()
    peer.feed(wire)
    assert h.reply.pending() == [(1, 0, 3), (3, 0, 3)]
    h.credit([window_update(1, 100) + window_update(3, 1)])
    h.receive(data(5, b"") + data(1, b"") + data(3, body(4, 1)) + data(1, b"", 1))
    wire, res = h.frame()
    peer.feed(wire)
    assert res[2] < 2 * res[0] and res[0] == 3 and h.reply.pending() == [(3, 0, 4), (5, 0, 3), (3, 4, 0)]
    drain(h, peer, [window_update(3, 100) + window_update(5, 100)])
    assert peer.got == {1: [b"", b"", b""], 3: [b"", body(4, 1)], 5: [b""]} and not peer.partial
    h.close()


def test_statuses_routes_and_a_routed_stream_with_its_own_window(gpu):
    # OK, TOO_LARGE, TRUNCATED and NO_SPACE in one call; stream 5 has no route; 3 -> 13 has a window of its own
    h = WH(gpu, streams=(1, 3, 5), routes={1: 11, 3: 13}, out_streams=(11, 13), arena_bytes=4096 + 256, max_msg=1200,
           initial_window=700)
    h.credit([window_update(13, 7)])
    h.receive(data(5, body(3, 1)) + _dropped_slices())
    statuses = [d[4] for d, _ in h.r.last]
    assert sorted(set(statuses)) == [0, 1, 2, 3] and statuses[0] == 0  # (every status is there; stream 5's is OK)
    kept = [b for d, b in h.r.last if d[4] == 0 and d[3] == 1]
    wire, res = h.frame()
    assert res[9] == len(statuses) - len(kept) - 1 and res[10] == 1 and res[11] == 0 and res[8] == len(kept)
    assert res[6] == STALL_STREAM and h.s.sw.windows([11, 13]) == [0, 707]
    assert h.releasable == 3  # (the unrouted one, the empty one, the dropped one; then the one the window cut)
    peer = Peer((11, 13))
    peer.feed(wire)
    h.release()
    drain(h, peer, [window_update(11, 5000)])
    assert peer.got[11] == kept and [len(b) for b in kept[:2]] == [0, 1000] and 13 not in peer.got
    h.release()
    assert h.r.asm.stats()["bytes_in_use"] == 0
    h.close()


def test_a_reset_between_two_calls_drops_the_partly_sent_entry(gpu):
    h = WH(gpu, initial_window=100, conn_window=65535)
    h.receive(data(3, body(50, 1)) + data(1, body(200, 2)) + data(1, body(10, 3)))
    wire, res = h.frame()
    assert res[:2] == (1, 2) and res[12] == 1 and h.reply.pending() == [(1, 200, 100), (1, 10, 0)]
    h.receive([rst(1)])
    wire, res = h.frame()
    assert res[:2] == (0, 0) and res[11] == 2 and wire == b"" and h.reply.pending() == []
    assert res[12] == 3  # (nothing refers to the ring any more)
    h.release()
    assert h.r.asm.stats()["bytes_in_use"] == 0
    h.close()


def test_settings_lower_the_frame_size_between_two_pieces(gpu):
    h = WH(gpu, initial_window=20000, conn_window=1 << 20, peer_max_frame=65536, max_frame=65536)
    peer = Peer((1, 3, 5), max_frame=65536)
    h.receive(data(1, body(40000, 1)))
    wire, res = h.frame()
    peer.feed(wire)
    assert res[2] == 2 and wire[:3] == (20000).to_bytes(3, "big")  # (one frame of the whole grant)
    h.credit([settings([(5, 16384)]) + window_update(1, 1 << 20)])
    wire, res = h.frame()
    peer.feed(wire)
    assert wire[:3] == (16384).to_bytes(3, "big") and res[2] == 4 and res[:2] == (1, 0)
    assert peer.got == {1: [body(40000, 1)]} and not peer.partial
    h.close()


def test_the_ring_wraps_over_what_was_released(gpu):
    # A finishes and is released; C lands on A's bytes; B's rest, cut before, still goes out right
    h = WH(gpu, arena_bytes=2048, initial_window=600, conn_window=65535)
    peer = Peer((1, 3, 5))
    h.receive(data(1, body(500, 1)) + data(3, body(1100, 2)))
    wire, res = h.frame()
    peer.feed(wire)
    assert res[:2] == (1, 1) and res[12] == 1 and h.r.model.bytes_in_use() == 1792
    h.release()
    assert h.r.model.bytes_in_use() == 1280
    got = h.receive(data(5, body(400, 3)))
    assert (got[0].status, got[0].offset) == (0, 0)  # (wrapped: where A lay)
    h.credit([window_update(3, 1000)])
    wire, res = h.frame()
    peer.feed(wire)
    assert res[:2] == (2, 0) and res[12] == 2
    assert peer.got == {1: [body(500, 1)], 3: [body(1100, 2)], 5: [body(400, 3)]} and not peer.partial
    h.release()
    assert h.r.asm.stats()["bytes_in_use"] == 0
    h.close()


def test_overflows_and_their_repeats(gpu):
    h = WH(gpu, initial_window=10, conn_window=65535, max_frame=16, max_pending=4)
    peer = Peer((1, 3, 5))
    h.credit([window_update(1, 1000) + window_update(3, 1000)])
    # the slice cap, then the header cap: nothing is written, no window moves, the source call is not taken
    h.receive(data(1, body(100, 1)) + data(3, body(100, 2)))
    wire, res = h.frame(cap=5)
    assert res[7] == 1 and res[2] == 28 and res[12] == 0
    wire, res = h.frame(cap=28, hdr_cap=32 * 9)
    assert res[7] == 1 and res[3] == 32 * 14
    wire, res = h.frame(cap=28)
    peer.feed(wire)
    assert res[7] == 0 and res[:2] == (2, 0) and res[8] == 2
    # the queue is full: three entries wait, two more arrive
    h.receive(data(5, body(30, 3)) + data(5, body(30, 4)) + data(5, body(30, 5)))
    wire, res = h.frame()
    peer.feed(wire)
    assert res[:2] == (0, 3)
    h.receive(data(1, body(30, 6)) + data(3, body(30, 7)))
    wire, res = h.frame()
    assert res[7] == 2 and res[1] == 5 and h.reply.pending() == [(5, 30, 10), (5, 30, 0), (5, 30, 0)]
    h.credit([window_update(5, 1000)])  # (a plain deframing: no source call)
    wire, res = h.frame(pending_only=True)
    peer.feed(wire)
    assert res[:2] == (3, 0) and res[8] == 0 and res[12] == 5  # (all but the source call that waits)
    wire, res = h.frame()
    peer.feed(wire)
    assert res[:2] == (2, 0) and res[8] == 2 and res[13] == 0
    assert peer.got == {1: [body(100, 1), body(30, 6)], 3: [body(100, 2), body(30, 7)], 5: [body(30, 3), body(30, 4), body(30, 5)]}
    h.close()


def test_4096_messages_on_2048_streams(gpu):
    # two one-byte messages per stream; every second stream's window ends behind its first (blocks and wave tiles crossed)
    ids = [2 * k + 1 for k in range(2048)]
    h = WH(gpu, streams=ids, table_slots=4096, arena_bytes=4096 * 256, initial_window=6, conn_window=MAXW, cap=8200)
    h.credit([b"".join(window_update(s, 6) for s in ids[i::8] if (s >> 1) & 1) for i in range(8)])
    frames = [frame(0, 0, s, grpc_msg(bytes([(s + r) & 0xff]))) for r in (0, 1) for s in ids]
    h.receive([b"".join(frames[i:i + 512]) for i in range(0, 4096, 512)])
    wire, res = h.frame()
    assert res[:2] == (3072, 1024) and res[5] == 6 * 3072 and res[6] == STALL_STREAM and res[12] == 2048
    assert h.reply.pending()[:2] == [(1, 1, 0), (5, 1, 0)]
    h.credit([b"".join(window_update(s, 6) for s in ids[i::8]) for i in range(8)])
    wire, res = h.frame()
    assert res[:2] == (1024, 0) and res[12] == 4096
    h.close()


def test_a_skipped_source_call(gpu):
    h = WH(gpu, streams=(1, 3), routes={1: 11}, out_streams=(11,), initial_window=100)
    h.receive(data(1, body(300, 1)))
    wire, res = h.frame()
    assert res[:2] == (0, 1)
    h.skipped_receive(data(1, body(10, 2)) + data(1, body(10, 3)), ev_cap=3)
    wire, res = h.frame()  # the call the assembler skipped: overflow 1, nothing is framed, the queue stands
    assert res[7] == 1 and res[2:5] == (0, 0, 0) and h.reply.pending() == [(11, 300, 100)]
    h.credit([window_update(11, 150)])
    wire, res = h.frame(pending_only=True)
    assert res[7] == 0 and h.reply.pending() == [(11, 300, 250)]
    h.receive(data(1, body(20, 4)))  # (the skipped call is lost with the next one)
    h.credit([window_update(11, 1000)])
    wire, res = h.frame()
    assert res[:2] == (2, 0) and res[13] == 1 and res[8] == 1
    h.close()


def test_a_send_windows_frame_call_between_two_replies(gpu):
    h = WH(gpu, initial_window=100, conn_window=400)
    peer = Peer((1, 3, 5))
    h.receive(data(1, body(200, 1)) + data(3, body(150, 2)))
    wire, res = h.frame()
    peer.feed(wire)
    assert h.reply.pending() == [(1, 200, 100), (3, 150, 100)]
    own = [(body(60, 9), 5, 0), (body(300, 8), 5, 0)]
    w5, r5, prog = h.s.frame(own, [0, 0], 16384)  # (the host's own messages under the same windows)
    peer.feed(w5)
    assert prog == [65, 35] and h.s.sw.windows([0, 5]) == [100, 0]
    h.credit([window_update(1, 70) + window_update(3, 70)])
    wire, res = h.frame()
    peer.feed(wire)
    assert res[6] == STALL_CONN | STALL_STREAM and h.reply.pending() == [(1, 200, 170), (3, 150, 130)]
    drain(h, peer, [window_update(0, 1000) + window_update(1, 1000) + window_update(3, 1000)])
    assert peer.got[1] == [body(200, 1)] and peer.got[3] == [body(150, 2)] and peer.got[5] == [body(60, 9)]
    h.close()


def test_echo_round_trip_with_the_clients_ledger(gpu):
    # RFC 7540's default windows on both sides: the server echoes three 200 000-byte messages under the client's
    # windows, the client's ledger returns the credit, the server takes it in and frames what waited
    bodies = [(1, body(200000, 1)), (3, body(200000, 2)), (1, body(200000, 3))]
    h = WH(gpu, streams=(1, 3), arena_bytes=1 << 20, cap=256)
    client = FH(gpu, streams=(1, 3), stream_window=65535, conn_window=65535, conn_threshold=0, max_updates=64)
    peer = Peer((1, 3))
    h.receive([f for s, b in bodies for f in data(s, b)])
    rounds, pending_only = 0, False
    while True:
        wire, res = h.frame(pending_only=pending_only)
        peer.feed(wire)
        sl, pos = [], 0
        for _, n in h.last_slices:
            sl.append(wire[pos:pos + n])
            pos += n
        h.release()
        rounds += 1
        if not h.model.queue:
            break
        res_c, back = client.feed(sl)
        assert res_c[5] == 0 and res_c[7] == 0
        h.credit([back])
        pending_only = True
        assert rounds < 100
    assert peer.got == {1: [bodies[0][1], bodies[2][1]], 3: [bodies[1][1]]} and not peer.partial
    assert rounds >= 600015 // 65535 and h.r.asm.stats()["bytes_in_use"] == 0
    client.close()
    h.close()


def test_refusals_and_lifetime(gpu):
    g = gpu
    from grpc_rdma_amd import h2dev
    h = WH(g, attach=False)
    t = g.DeviceBuffer(nbytes=8192)
    ok = (t.ptr, 8, t.ptr + 4096, 128)
    with pytest.raises(g.GrdmaError, match="no send windows attached"):
        h.reply.frame_windowed(*ok)
    for n in (0, 4097):
        with pytest.raises(g.GrdmaError, match="max_pending"):
            h.reply.attach_windows(h.s.sw, n)
    h.reply.attach_windows(h.s.sw, 8)
    with pytest.raises(g.GrdmaError, match="attached already"):
        h.reply.attach_windows(h.s.sw, 8)
    other = h2dev.Reply(h.r.asm, None, 16384)
    with pytest.raises(g.GrdmaError, match="attached to a reply already"):
        other.attach_windows(h.s.sw, 8)
    other.close()
    with pytest.raises(g.GrdmaError, match="no source call yet"):
        h.reply.frame_windowed(*ok)
    h.receive(data(1, body(10, 1)))
    with pytest.raises(g.GrdmaError):  # (one message could go out twice)
        h.reply.frame(*ok)
    assert b"frames under send windows" in h2dev.load().grdma_last_error()
    for args, why in (((t.ptr + 8, 8, t.ptr + 4096, 128), "misaligned"), ((t.ptr, 0, t.ptr + 4096, 128), "misaligned"),
                      ((t.ptr, 8, 0, 128), "misaligned"), ((t.ptr, 8, t.ptr + 4100, 128), "misaligned")):
        with pytest.raises(g.GrdmaError, match=why):
            h.reply.frame_windowed(*args)
    out = (h2dev.u64 * 16)()
    assert h2dev.load().grdma_h2_reply_frame_windowed(h.reply.h, 2, t.ptr, 8, t.ptr + 4096, 128, out) == -2
    sl, st = h.reply.frame_windowed(*ok)  # (the refusals left it working)
    assert st["finished"] == 1 and st["releasable"] == 1 and len(sl) == 2
    # the send windows destroyed first: the reply refuses every call and can still be closed
    h.s.sw.close()
    with pytest.raises(g.GrdmaError, match="send windows are gone"):
        h.reply.frame_windowed(*ok)
    with pytest.raises(g.GrdmaError):
        h.reply.frame(*ok)
    h.reply.close()
    assert h.reply.h is None
    # the reply destroyed first: the send windows refuse every call and can still be closed
    sw = h2dev.SendWindows(h.r.parser)
    reply = h2dev.Reply(h.r.asm, None, 16384)
    reply.attach_windows(sw, 8)
    reply.close()
    with pytest.raises(g.GrdmaError, match="reply framer .* is gone"):
        sw.frame([(t.ptr, 4, 1, 0)], [0], 16, t.ptr, 8, t.ptr + 4096, 128)
    with pytest.raises(g.GrdmaError, match="reply framer .* is gone"):
        sw.intake()
    other = h2dev.Reply(h.r.asm, None, 16384)
    with pytest.raises(g.GrdmaError, match="attached to a reply already"):
        other.attach_windows(sw, 8)
    sw.close()
    # a parser that is gone, a reply bound to a reply pipe's kind of source: the attachment is refused
    p2 = h2dev.Parser(False)
    sw2 = h2dev.SendWindows(p2)
    p2.close()
    with pytest.raises(g.GrdmaError, match="parser is gone"):
        other.attach_windows(sw2, 8)
    sw2.close()
    other.close()
    h.r.close()
