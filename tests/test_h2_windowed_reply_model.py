"""tests/h2_windowed_reply_model.py pinned before a device test trusts it (CPU, no device): under open windows against
the oracle's framing of what the assembler's model kept, and on seeded random runs of {receive, credit, reply, release}
end to end through an oracle parser, against an independent count of the bytes the peer allowed, and against the
assembler model's ring."""
import random
import struct

import pytest

from oracle import pyorc
from tests.h2_asm_model import OK, AsmModel
from tests.h2_device_lib import _client_stream, _eight_streams, expected_reply, oracle_feed
from tests.h2_helpers import frame, grpc_msg
from tests.h2_send_model import MAXW, SendModel, live_of
from tests.h2_windowed_reply_model import LOST, WindowedReplyModel

BIG = 1 << 40


def test_the_entry_points_exist(built):
    """(what makes every test of this file fail on a tree without the feature: the model describes calls that are there)"""
    from grpc_rdma_amd import h2dev
    lib = h2dev.load()
    assert all(hasattr(lib, n) for n in ("grdma_h2_reply_attach_windows", "grdma_h2_reply_frame_windowed",
                                         "grdma_h2_reply_frame_windowed_batch", "grdma_h2_reply_pending"))
    assert h2dev.Reply.WINDOWED[12] == "releasable" and len(h2dev.Reply.WINDOWED) == 16


@pytest.mark.parametrize("routed", [False, True])
def test_open_windows_equal_expected_reply(routed):
    cases = [(True, _eight_streams(s, nmsg=3)[1], ()) for s in (1, 2, 3)]
    cases += [(False, [w[i:i + 7000] for i in range(0, len(w), 7000)], (1, 3, 5)) for w in (_client_stream(s, [1, 3, 5], 12) for s in (4, 5))]
    for mf in (16384, 100, 5):
        for prefix, calls, streams in cases:
            orc = pyorc.H2Parser(prefix)
            for s in streams:
                assert orc.open_stream(s) == 0
            routes = {s: s + 100 for s in (1, 3, 7, 9)} if routed else None
            out = orc if not routed else pyorc.H2Parser(False)  # (a proxy: the replies go out on another transport)
            if routed:
                for s in routes.values():
                    assert out.open_stream(s) == 0
            asm = AsmModel(1 << 30)
            wr = WindowedReplyModel(asm, SendModel(MAXW, MAXW, (1 << 24) - 1), mf, routes)
            for slices in calls:
                err, ev = oracle_feed(orc, [slices])
                assert err == 0
                reported = asm.call(ev, [slices], 0)
                wr.source_call(reported)
                lens, wire, res = wr.frame(live_of(out), BIG, BIG)
                wire_o, lens_o, counters = expected_reply(reported, mf, routes)
                assert (wire, lens) == (wire_o, lens_o)
                assert res[:2] == (counters["kept"], 0) and res[2] == len(lens) and res[4] == len(wire)
                assert res[5] == sum(5 + len(b) for (d, b) in reported if d[4] == OK and (routes is None or d[3] in routes))
                assert res[6:12] == (0, 0, counters["kept"], counters["dropped_status"], counters["unrouted"], 0)
                assert res[12] == len(reported) and res[13] == 0 and wr.queue == []
                asm.release(res[12])
                assert asm.released == asm.reported


def data_frames(wire):
    """the DATA frames of a wire, read without the library or the oracle -> [(stream, payload)]"""
    out, o = [], 0
    while o < len(wire):
        n, t, sid = int.from_bytes(wire[o:o + 3], "big"), wire[o + 3], int.from_bytes(wire[o + 5:o + 9], "big")
        assert t == 0 and n > 0 and o + 9 + n <= len(wire)
        out.append((sid, wire[o + 9:o + 9 + n]))
        o += 9 + n
    return out


def run(seed):
    """one seeded run -> nothing; every property is asserted on the way"""
    rng = random.Random(seed)
    sids = [1, 3, 5, 7]
    iws, conn0 = rng.choice((0, 3, 5, 6, 40, 300)), rng.choice((0, 7, 60, 500))
    server = pyorc.H2Parser(False)   # the transport that receives the requests and sends the echoes
    client = pyorc.H2Parser(False)   # the peer: fed the concatenated echo wires
    for s in sids:
        assert server.open_stream(s) == 0 and client.open_stream(s) == 0
    asm = AsmModel(1 << 16, max_message_bytes=600, max_pending=rng.choice((3, 64)))
    send = SendModel(iws, conn0, 16384)
    max_pending = rng.choice((4, 4096))
    wr = WindowedReplyModel(asm, send, rng.choice((5, 6, 23, 100, 16384)), None, max_pending)
    allowed = {s: iws for s in sids}   # the independent counter: what the peer has allowed, what was sent
    allowed[0] = conn0
    sent = dict.fromkeys([0] + sids, 0)
    want = {s: [] for s in sids}       # the kept messages per stream, in the order they were reported
    reset, got, partial = set(), {s: [] for s in sids}, {}
    releasable = 0
    new_since_reply = 0
    lost_expected = False

    def receive(parts):
        nonlocal new_since_reply, lost_expected
        err, ev = oracle_feed(server, parts)
        assert err == 0
        reported = asm.call(ev, parts, 0)
        wr.source_call(reported)
        send.intake(ev, parts, 0, live_of(server))
        new_since_reply += 1
        if new_since_reply > 1:
            lost_expected = True
        return reported

    def reply(pending_only=False):
        nonlocal releasable, new_since_reply
        taking = wr.new if (wr.calls > wr.taken and not pending_only) else None
        before = asm.reported
        lens, wire, res = wr.frame(live_of(server), BIG, BIG, pending_only)
        if res[7] == 2:  # the queue is full: nothing was written; credit, then the queue alone
            assert (lens, wire) == ([], b"") and res[1] > max_pending
            return res
        assert res[7] == 0 and sum(lens) == len(wire) == res[4] and not (res[6] & 4)
        if taking is not None:
            new_since_reply = 0
            for d, body in taking[0]:
                if d[4] == OK and d[3] in live_of(server):
                    want[d[3]].append(body)
        assert (res[13] == LOST) == wr.lost and (not wr.lost or lost_expected)
        for sid, pay in data_frames(wire):
            sent[sid] += len(pay)
            sent[0] += len(pay)
            assert sent[sid] <= allowed[sid], "stream %d: %d bytes sent, %d allowed" % (sid, sent[sid], allowed[sid])
            assert sent[0] <= allowed[0], "connection: %d bytes sent, %d allowed" % (sent[0], allowed[0])
        rc, ev = client.feed(wire)
        assert rc == 0
        for k, a, b, c, d in ev:
            if k == pyorc.EV_MSG_BEGIN:
                partial[c] = bytearray()
            elif k == pyorc.EV_MSG_BYTES:
                partial[c] += wire[a:a + b]
            elif k == pyorc.EV_MSG_END:
                got[c].append(bytes(partial.pop(c)))
        # (d) releasable never covers a pending entry, nor a source call that is still to be taken
        releasable = res[12]
        assert all(e.rank >= asm.released + releasable for e in wr.queue)
        if wr.calls > wr.taken:
            assert asm.released + releasable <= wr.new[1]
        assert asm.released + releasable <= before == asm.reported
        return res

    for step in range(rng.randrange(4, 30)):
        what = rng.choice(("receive", "receive", "credit", "reply", "reply", "release", "reset"))
        livenow = sorted(live_of(server))
        if what == "receive" and livenow:
            parts = []
            for _ in range(rng.randrange(1, 5)):
                s = rng.choice(livenow)
                body = grpc_msg(bytes(rng.getrandbits(8) for _ in range(rng.choice((0, 0, 1, 4, 9, 30, 200, 700)))), rng.randrange(2))
                cut = rng.randrange(0, len(body) + 1)
                parts += [frame(0, 0, s, body[:cut]), frame(0, 0, s, body[cut:])] if 0 < cut < len(body) else [frame(0, 0, s, body)]
            receive(parts)
        elif what == "credit":
            parts = []
            for _ in range(rng.randrange(1, 4)):
                s, inc = rng.choice([0] + sids), rng.choice((1, 2, 5, 9, 50, 400))
                parts.append(frame(8, 0, s, struct.pack(">I", inc)))
                if s == 0 or s in live_of(server):
                    allowed[s] += inc
            receive(parts)
        elif what == "reset" and len(livenow) > 1:
            s = rng.choice(livenow)
            receive([frame(3, 0, s, (8).to_bytes(4, "big"))])
            reset.add(s)
            assert s not in live_of(server)
        # (mostly a reply behind every source call: a call that is never taken is LOST, and the flag is sticky)
        if (what == "reply" or (new_since_reply and rng.randrange(8))) and wr.calls:
            res = reply(rng.randrange(8) == 0)
            if res[7] == 2:
                receive([frame(8, 0, s, struct.pack(">I", 100000)) for s in [0] + sorted(live_of(server))])
                for s in [0] + sorted(live_of(server)):
                    allowed[s] += 100000
                res = reply(True)
                assert res[7] == 0
        elif what == "release":
            asm.release(releasable)
            releasable = 0
            assert all(e.rank >= asm.released for e in wr.queue)
            # the ring still holds every pending entry's record: the tail has not passed one
            held = {r[2] for r in asm.recs.values()}
            assert all(e.rank in held for e in wr.queue if len(e.body))
    # drain: the peer opens its windows, the queue empties in as many calls as the model needs
    for _ in range(4):
        receive([frame(8, 0, s, struct.pack(">I", 1 << 20)) for s in [0] + sorted(live_of(server))])
        for s in [0] + sorted(live_of(server)):
            allowed[s] += 1 << 20
        res = reply()
        if res[7] == 0 and res[1] == 0:
            break
    assert wr.queue == [] and res[7] == 0
    # (b) whole, once, in per-stream order: exactly so on a stream that stayed; a reset stream got a prefix, the later
    # ones dropped (a source call that was lost took its messages with it: they were never in `want`)
    for s in sids:
        if s in reset:
            assert got[s] == want[s][:len(got[s])], (seed, s)
        else:
            assert got[s] == want[s] and s not in partial, (seed, s, len(got[s]), len(want[s]))
    asm.release(res[12])
    assert asm.released == asm.reported and asm.bytes_in_use() == 0


def test_two_thousand_random_runs():
    for seed in range(2000):
        run(seed)


def test_one_more_would_free_a_pending_message():
    """releasable is exact: released one further, the assembler's ring gives up the oldest pending entry's record"""
    server = pyorc.H2Parser(False)
    assert server.open_stream(1) == 0
    asm = AsmModel(1 << 16)
    wr = WindowedReplyModel(asm, SendModel(100, 1000, 16384), 16384)
    parts = [frame(0, 0, 1, grpc_msg(b"a" * 50)), frame(0, 0, 1, grpc_msg(b"b" * 200)), frame(0, 0, 1, grpc_msg(b"c" * 10))]
    err, ev = oracle_feed(server, parts)
    wr.source_call(asm.call(ev, parts, err))
    lens, wire, res = wr.frame(live_of(server), BIG, BIG)
    assert res[:2] == (1, 2) and res[5] == 100 and res[12] == 1 and wr.pending() == [(1, 200, 45), (1, 10, 0)]
    asm.release(1)
    assert asm.bytes_in_use() == 256 + 256 and wr.queue[0].rank == 1
    asm.release(1)  # one more
    assert asm.bytes_in_use() == 256, "the record of the entry that is partly sent is gone"
