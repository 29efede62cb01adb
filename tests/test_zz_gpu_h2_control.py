"""Control replies on the device: SETTINGS ACK, PING ACK and RST_STREAM written from a deframing's events, and the record
of what the peer said (grdma_h2_ctl, csrc/grdma_h2_ctl.h).  The expected values come from the ControlModel of
tests/h2_control_model.py: the rules of include/grdma_amd.h applied to the ORACLE's event list and the bytes fed.  Every
comparison is exact (CH of tests/h2_control_lib.py runs a call on the device and in the model and compares slices, the
whole slice table and header arena, result block, peer record and counters)."""
import pytest

from tests.h2_control_lib import CH, ERR5, Target, bad_flags, bad_grpc, cut_at, data, goaway, ping, settings
from tests.h2_control_model import GOAWAY, LOST, SETTINGS_ACK, ControlModel, ping_ack, rst_stream
from tests.h2_device_lib import FH, same
from tests.h2_helpers import PREFACE, frame, grpcio_capture
from tests.h2_send_lib import window_update
from tests.h2_send_model import SendModel, live_of

pytestmark = pytest.mark.gpu

MIXED = (settings(2) + ping(0x0102030405060708) + data(1) + bad_flags(3) + ping(0xa1a2a3a4a5a6a7a8) + settings(0) + data(5) +
         goaway(7, 2, b"bye") + ping(0x1112131415161718, ack=True) + settings(ack=True) + bad_flags(5, 0) + settings(1) + ping(3))


def test_whole_frames_of_each_kind(gpu):
    h = CH(gpu, streams=(1, 3, 5))
    wire, res = h.feed([MIXED])
    assert res == (8, 5, 3 * 17 + 3 * 9 + 2 * 13, 3, 3, 2, GOAWAY, 0)
    assert wire == (ping_ack(bytes(range(1, 9))) + ping_ack(bytes(range(0xa1, 0xa9))) + ping_ack((3).to_bytes(8, "big")) +
                    SETTINGS_ACK + rst_stream(3) + SETTINGS_ACK + rst_stream(5) + SETTINGS_ACK)
    assert h.model.peer == dict(settings_acks=1, ping_acks=1, last_ping_opaque=0x1817161514131211, goaways=1, goaway_last_stream=7,
                                goaway_error=2, goaway_call=1)
    h.close()


def test_one_byte_slices(gpu):
    h = CH(gpu, streams=(1, 3, 5))
    wire, res = h.feed([MIXED[i:i + 1] for i in range(len(MIXED))])
    assert res[:6] == (8, 5, 104, 3, 3, 2)
    h.close()


def test_the_grpcio_capture(gpu):
    capture, _ = grpcio_capture()
    h = CH(gpu, prefix=True)
    wire, res = h.feed([capture])
    assert (wire, res) == (SETTINGS_ACK, (1, 1, 9, 1, 0, 0, 0, 0)) and h.model.peer["settings_acks"] == 1
    h.close()
    # ... cut inside the SETTINGS frame's header and payload: the ACK is due with the frame's last byte
    first = len(PREFACE)
    for at in (first + 4, first + 9, first + 9 + 35):
        h = CH(gpu, prefix=True)
        assert h.feed([capture[:at]])[1][:3] == (0, 0, 0)
        assert h.feed([capture[at:]]) == (SETTINGS_ACK, (1, 1, 9, 1, 0, 0, 0, 0))
        h.close()


@pytest.mark.parametrize("cut", [4, 9, 10, 16, 17])
def test_ping_cut_between_calls(gpu, cut):
    # inside the 9-byte header, and after 0, 1, 7 and 8 payload bytes (the last: behind the frame)
    h = CH(gpu, streams=(1,))
    w = settings(1) + ping(0x0807060504030201) + ping(0xf1f2f3f4f5f6f7f8, ack=True) + ping(0x2122232425262728)
    for first, at in ((True, 15 + cut), (False, 15 + 17 + cut)):  # the PING, then the PING ACK behind it
        a, b = h.feed([w[:at]]), h.feed(cut_at(w[at:], 1, 2))
        pings_a = 1 if cut == 17 else 0
        if first:
            assert a[1][:6] == (1 + pings_a, 1 if pings_a == 0 else 2, 9 + 17 * pings_a, 1, pings_a, 0)
            assert b[1][4] == 2 - pings_a and b[0].startswith(ping_ack((0x2122232425262728 if pings_a else 0x0807060504030201).to_bytes(8, "big")))
            assert h.model.peer["last_ping_opaque"] == 0xf8f7f6f5f4f3f2f1
        else:
            assert a[1][4] == 1 and b[1][4] == 1 and h.model.peer["ping_acks"] == 2
    # a frame cut twice: a call that delivers one byte of it
    p = ping(0x3132333435363738)
    assert h.feed([p[:12]])[1][0] == 0 and h.feed([p[12:13]])[1][0] == 0
    assert h.feed([p[13:]])[0] == ping_ack(p[9:])
    h.close()


@pytest.mark.parametrize("cut", [4, 9, 10, 16, 17, 30, 57])
def test_settings_and_goaway_cut_between_calls(gpu, cut):
    # the cut falls inside the 9-byte header, after 0, 1, 7 and 8 payload bytes and, in the GOAWAY, inside its 40 bytes
    # of debug data and behind the frame
    h = CH(gpu, streams=(1,))
    s = settings(3)  # (18 bytes of payload)
    if cut <= 9 + 18:
        w = ping(1) + s + ping(2)
        a, b = h.feed([w[:17 + cut]]), h.feed([w[17 + cut:]])
        assert (a[1][3], b[1][3]) == ((1, 0) if cut == 27 else (0, 1)) and a[1][4] == b[1][4] == 1
    g = goaway(0x80000009, 0xcafe0102, bytes(range(40)))
    w = goaway(1, 1) + g + settings(ack=True)
    a = h.feed([w[:17 + cut]])
    assert a[1][6] == GOAWAY and h.model.peer["goaway_last_stream"] == (9 if cut == 57 else 1)
    b = h.feed(cut_at(w[17 + cut:], 1))
    assert b[1][6] == (0 if cut == 57 else GOAWAY)
    assert (h.model.peer["goaways"], h.model.peer["goaway_last_stream"], h.model.peer["goaway_error"]) == (2, 9, 0xcafe0102)
    assert h.model.peer["goaway_call"] == h.model.stats["calls"] - (1 if cut == 57 else 0) and h.model.peer["settings_acks"] == 1
    h.close()


def test_zero_length_settings_and_what_the_peer_acknowledged(gpu):
    h = CH(gpu)
    assert h.feed([settings(0) + settings(0)]) == (SETTINGS_ACK * 2, (2, 1, 18, 2, 0, 0, 0, 0))
    # SETTINGS ACK and PING ACK from the peer: no reply, the counters move, the last opaque value is recorded
    wire, res = h.feed([settings(ack=True) + ping(0x0a0b0c0d0e0f1011, ack=True) + ping(0x99, ack=True) + settings(ack=True)])
    assert (wire, res) == (b"", (0, 0, 0, 0, 0, 0, 0, 0))
    assert h.model.peer == dict(settings_acks=2, ping_acks=2, last_ping_opaque=0x99 << 56, goaways=0, goaway_last_stream=0,
                                goaway_error=0, goaway_call=0)
    h.close()


def test_two_goaways_in_one_call(gpu):
    h = CH(gpu)
    h.feed([ping(1)])
    wire, res = h.feed([goaway(11, 1, b"first"), ping(5), goaway(3, 0xb)])
    assert res == (1, 1, 17, 0, 1, 0, GOAWAY, 0)
    assert (h.model.peer["goaways"], h.model.peer["goaway_last_stream"], h.model.peer["goaway_error"], h.model.peer["goaway_call"]) == (2, 3, 0xb, 2)
    h.close()


def test_order_of_interleaved_replies(gpu):
    h = CH(gpu, streams=(1, 3, 5, 7))
    w = (bad_flags(5) + ping(1) + settings(1) + data(1) + bad_grpc(3, good=2, tail=30) + ping(2) + bad_flags(1) + settings(0) +
         bad_grpc(7, good=0) + ping(3) + data(7) + bad_flags(7))
    # the DATA frame with the bad gRPC byte spread over several slices: the pseudo frame falls inside its payload run
    at = w.index(bad_grpc(3, good=2, tail=30))
    wire, res = h.feed(cut_at(w, at + 12, at + 20, at + 24, at + 40))
    assert wire == (ping_ack((1).to_bytes(8, "big")) + ping_ack((2).to_bytes(8, "big")) + ping_ack((3).to_bytes(8, "big")) +
                    rst_stream(5) + SETTINGS_ACK + rst_stream(3) + rst_stream(1) + SETTINGS_ACK + rst_stream(7) + rst_stream(7))
    assert res == (10, 6, 51 + 18 + 65, 2, 3, 5, 0, 0)  # (stream 7 twice: the writer does not deduplicate)
    h.close()


@pytest.mark.parametrize("lead", [(), (settings(1),), (bad_flags(3), settings(1))])
def test_replies_spanning_workgroup_shares(gpu, lead):
    # 600 PINGs between DATA frames: replies fall into several workgroups' shares (into both of the emulator's grid); with
    # 0, 9 and 22 bytes queued in front the 23-byte cuts fall inside PINGs' opaque bytes and inside a RST_STREAM
    h = CH(gpu, streams=(1, 3, 5), cap=600)
    frames = list(lead)
    for k in range(600):
        frames += [ping(0x0100000000000000 * (k % 251) + k), data(1, bytes(k % 7))]
        if k % 97 == 5:
            frames.append(settings(k % 3))
        if k == 300:
            frames.append(bad_flags(5))
    w = b"".join(frames)
    wire, res = h.feed(cut_at(w, len(w) // 3, len(w) // 3 + 1, len(w) - 20), ev_cap=16384)
    assert res[4] == 600 and res[5] == len(lead[:-1]) + 1 and res[1] == -(-res[2] // 23)
    cuts = {o % 17 if o < 600 * 17 else "queued" for o in range(23, res[2], 23)}
    assert {9, 10, 16}.issubset(cuts)  # (cuts behind the PING ACK's header, inside and behind its opaque bytes)
    h.close()


def test_no_control_frame_at_all(gpu):
    h = CH(gpu, streams=(1,))
    assert h.feed([data(1) + window_update(1, 5) + data(1, b"x" * 40)]) == (b"", (0, 0, 0, 0, 0, 0, 0, 0))
    h.target.untouched("a call without control frames")
    assert h.feed([]) == (b"", (0, 0, 0, 0, 0, 0, 0, 0))
    h.close()


def test_connection_error_in_the_call(gpu):
    h = CH(gpu, streams=(1,))
    p = ping(0x0102030405060708)
    assert h.feed([settings(1) + p[:12]])[1][:4] == (1, 1, 9, 1)
    err, _ = h.deframe([p[12:] + ping(7) + frame(6, 0, 0, b"short") + ping(9)])
    assert err == 15
    assert h.reply() == (b"", (0, 0, 0, 0, 0, 0, 0, 0))  # nothing written, taken, the carry dropped
    h.target.untouched("a call with a connection error")
    with pytest.raises(gpu.GrdmaError, match="taken in already"):
        h.ctl.reply(h.target.slices.ptr, 4, h.target.hdr.ptr, 128)
    assert h.model.carry is None and h.model.stats["ping_acks"] == 0
    h.close()


def test_lost_calls(gpu):
    # an event overflow: the sticky flag, -GRDMA_ERR_CAPACITY, overflow word 2, the carry goes
    h = CH(gpu)
    h.feed([ping(1) + ping(2)[:11]])
    with pytest.raises(gpu.GrdmaError, match=ERR5):
        h.deframe([ping(2)[11:]] + [ping(3)] * 40, ev_cap=16, checked=False)
    t = Target(gpu, 8)
    with pytest.raises(gpu.GrdmaError, match=ERR5):
        h.ctl.reply(t.slices.ptr, 8, t.hdr.ptr, 256)
    same(h.ctl.last_result, h.model.lost_call()[2], "the lost call's result")
    assert h.ctl.last_result == (0, 0, 0, 0, 0, 0, LOST, 2)
    t.untouched("a lost call")
    h.check()
    with pytest.raises(gpu.GrdmaError, match="taken in already"):
        h.ctl.reply(t.slices.ptr, 8, t.hdr.ptr, 256)
    h.close()
    # a standalone deframing that was never taken in: the flag in every later result block, the carry dropped, the later
    # calls exact apart from the flag
    h = CH(gpu, streams=(1,))
    h.feed([ping(1) + ping(0x0102030405060708)[:13]])
    h.deframe([ping(0x0102030405060708)[13:] + ping(4)])  # (never taken in)
    h.skipped = True
    p = ping(0x2122232425262728)
    wire, res = h.feed([settings(1) + bad_flags(1) + p[:10]])
    assert (wire, res) == (SETTINGS_ACK + rst_stream(1), (2, 1, 22, 1, 0, 1, LOST, 0))
    wire, res = h.feed([p[10:]])
    assert (wire, res) == (ping_ack(p[9:]), (1, 1, 17, 0, 1, 0, LOST, 0)) and h.ctl.stats()["lost"]
    h.close()


@pytest.mark.parametrize("short", ["max_replies", "slices", "header"])
def test_cap_overflow_then_repeat(gpu, short):
    # nothing written, nothing committed, not taken; the repeated call with larger targets is the model's single call,
    # with a cut PING pending in the carry
    h = CH(gpu, streams=(1,), max_replies=4 if short == "max_replies" else 5)
    p, q = ping(0x0102030405060708), ping(0x1112131415161718)
    h.feed([goaway(5, 1) + settings(ack=True) + p[:14]])
    before = (dict(h.model.peer), dict(h.model.stats), dict(h.model.carry))
    h.deframe([p[14:] + settings(1) + bad_flags(1) + goaway(3, 9) + ping(2, ack=True) + ping(3) + settings(0) + q[:11]])
    # 5 replies, 17 + 17 + 9 + 13 + 9 = 65 bytes, 3 slices
    if short == "max_replies":
        wire, res = h.reply(cap=8)
        assert res == (5, 3, 65, 2, 2, 1, GOAWAY, 1)
        with pytest.raises(gpu.GrdmaError, match=ERR5):  # (max_replies is the writer's: the call stays unanswerable)
            h.ctl.reply(h.target.slices.ptr, 8, h.target.hdr.ptr, 256)
        assert (h.model.peer, h.model.stats, h.model.carry) == before
        h.check()
        h.close()
        return
    wire, res = h.reply(cap=2 if short == "slices" else 3, hdr_cap=95 if short == "header" else 96)
    assert res == (5, 3, 65, 2, 2, 1, GOAWAY, 1) and (h.model.peer, h.model.stats, h.model.carry) == before
    wire, res = h.reply(cap=3, hdr_cap=96)
    assert res == (5, 3, 65, 2, 2, 1, GOAWAY, 0)
    assert wire == ping_ack(p[9:]) + ping_ack((3).to_bytes(8, "big")) + SETTINGS_ACK + rst_stream(1) + SETTINGS_ACK
    assert h.model.peer["goaway_last_stream"] == 3 and h.model.peer["last_ping_opaque"] == 2 << 56 and h.model.carry["type"] == 6
    with pytest.raises(gpu.GrdmaError, match="taken in already"):
        h.ctl.reply(h.target.slices.ptr, 3, h.target.hdr.ptr, 96)
    assert h.feed([q[11:]])[0] == ping_ack(q[9:])
    h.close()


@pytest.mark.parametrize("first", ["writer", "others"])
def test_ledger_and_send_windows_on_the_same_deframing(gpu, first):
    from grpc_rdma_amd import h2dev
    f = FH(gpu, streams=(1, 3), stream_window=1 << 16, conn_window=1 << 16)
    ctl, cm = h2dev.ControlReplies(f.parser), ControlModel()
    sw, sm = h2dev.SendWindows(f.parser), SendModel()
    p = ping(0x0102030405060708)
    calls = ([data(1, b"x" * 300) + window_update(1, 77) + settings(1) + p[:12]],
             [p[12:] + window_update(0, 5) + data(3, b"y" * 500) + bad_flags(3) + frame(4, 0, 0, (4).to_bytes(2, "big") + (70000).to_bytes(4, "big"))])
    for slices in calls:
        f.deframe_checked(slices)
        err_o, ev_o = f.last
        t = Target(gpu, 8)

        def writer():
            lens, wire, res = cm.reply(ev_o, slices, err_o, 8, 256)
            sl, got = ctl.reply(t.slices.ptr, 8, t.hdr.ptr, 256)
            same(got, res, "writer: result")
            t.check(gpu, sl, lens, wire, "writer")

        def others():
            f.account()
            same(sw.intake(), sm.intake(ev_o, slices, err_o, live_of(f.pp.orc)), "intake: result")

        for step in ((writer, others) if first == "writer" else (others, writer)):
            step()
    assert cm.stats["ping_acks"] == 1 and cm.stats["settings_acks"] == 2 and cm.stats["rst_streams"] == 1 and sm.iws == 70000
    f.check_stats()
    same(sw.windows([0, 1]), [sm.window(0), sm.window(1)], "windows")
    ctl.close()
    sw.close()
    f.close()


def test_refusals_and_lifetime(gpu):
    from grpc_rdma_amd import h2dev
    h = CH(gpu)
    t = Target(gpu, 4)
    with pytest.raises(gpu.GrdmaError, match="already"):
        h2dev.ControlReplies(h.parser)
    for bad in (0, (1 << 24) + 1):
        p2 = h2dev.Parser(False, 16384)
        with pytest.raises(gpu.GrdmaError, match="max_replies"):
            h2dev.ControlReplies(p2, bad)
        h2dev.ControlReplies(p2, 1 << 24).close()
        p2.close()
    with pytest.raises(gpu.GrdmaError, match="deframed nothing"):
        h.ctl.reply(t.slices.ptr, 4, t.hdr.ptr, 128)
    h.deframe([ping(1)])
    for args in ((0, 4, t.hdr.ptr, 128), (t.slices.ptr, 0, t.hdr.ptr, 128), (t.slices.ptr, 4, 0, 128), (t.slices.ptr, 4, t.hdr.ptr, 0),
                 (t.slices.ptr + 8, 4, t.hdr.ptr, 128), (t.slices.ptr, 4, t.hdr.ptr + 4, 128)):
        with pytest.raises(gpu.GrdmaError, match="null, zero or misaligned"):
            h.ctl.reply(*args)
    t.untouched("refused calls")
    sl, res = h.ctl.reply(t.slices.ptr, 4, t.hdr.ptr, 128)  # (nothing changed: the call is still to be answered)
    assert res == (1, 1, 17, 0, 1, 0, 0, 0) and h.ctl.stats()["calls"] == 1
    with pytest.raises(gpu.GrdmaError, match="taken in already"):
        h.ctl.reply(t.slices.ptr, 4, t.hdr.ptr, 128)
    # a parser that is gone: every call is refused, destroy still works
    h.parser.close()
    with pytest.raises(gpu.GrdmaError, match="parser is gone"):
        h.ctl.reply(t.slices.ptr, 4, t.hdr.ptr, 128)
    assert h.ctl.peer()["ping_acks"] == 0 and h.ctl.stats()["ping_acks"] == 1
    h.ctl.close()
    h.ctl.close()
