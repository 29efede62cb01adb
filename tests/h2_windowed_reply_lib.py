"""The harness of the windowed reply's device tests (tests/test_zz_gpu_h2_windowed_reply.py, the many-link file beside
it): a source transport with its assembler (RHarness), the send windows of the transport the replies go out on (SH: the
source's own parser for an echo, another one for a proxy), an h2dev.Reply attached to them, and the model of
tests/h2_windowed_reply_model.py beside them.  Every call runs on the device and in the model and is compared exactly:
slice list, whole slice table and header arena with the fill outside the written part, result block, windows, the
queue's progress, the assembler's bytes in use.  pytest rewrites no `assert` in a helper module, so every check here goes
through `same`."""
import pytest

from oracle import pyorc
from tests.h2_device_lib import SENTINEL, RHarness, read_slices, same
from tests.h2_helpers import frame, grpc_msg
from tests.h2_send_lib import SH
from tests.h2_send_model import SendModel
from tests.h2_windowed_reply_model import WORDS, WindowedReplyModel


def data(sid, payload, compressed=0):
    """one gRPC message as DATA frames of at most 16384 bytes"""
    m = grpc_msg(payload, compressed)
    return [frame(0, 0, sid, m[o:o + 16384]) for o in range(0, len(m), 16384)]


def rst(sid):
    return frame(3, 0, sid, (8).to_bytes(4, "big"))


class Peer:
    """the peer's parser (the oracle's), fed the wires in order -> the messages per stream"""

    def __init__(self, streams, max_frame=16384):
        self.orc = pyorc.H2Parser(False, max_frame_size=max_frame)
        for s in streams:
            same(self.orc.open_stream(s), 0, "the peer's open_stream(%d)" % s)
        self.got, self.partial = {}, {}

    def feed(self, wire):
        rc, ev = self.orc.feed(wire)
        same(rc, 0, "the peer's parser over the wire")
        for k, a, b, c, d in ev:
            if k == pyorc.EV_MSG_BEGIN:
                self.partial[c] = bytearray()
            elif k == pyorc.EV_MSG_BYTES:
                self.partial[c] += wire[a:a + b]
            elif k == pyorc.EV_MSG_END:
                self.got.setdefault(c, []).append(bytes(self.partial.pop(c)))


def drain(h, peer, credit, limit=50):
    """credit, then the queue alone, until nothing waits -> the calls it took"""
    calls = 0
    while h.model.queue:
        h.credit(credit)
        wire, res = h.frame(pending_only=True)
        peer.feed(wire)
        calls += 1
        same(calls < limit, True, "the queue drains in fewer than %d calls" % limit)
    return calls


class SHOn(SH):
    """SH over a ParserPair that exists: the send windows of the source's own parser (an echo)"""

    def __init__(self, g, pp, streams, initial_window, conn_window, peer_max_frame):
        from grpc_rdma_amd import h2dev
        self.g, self.h2dev, self.pp = g, h2dev, pp
        self.parser = pp.dev
        self.sw = h2dev.SendWindows(self.parser, initial_window, conn_window, peer_max_frame)
        self.model = SendModel(initial_window, conn_window, peer_max_frame)
        self.named = set(streams)
        self.last, self.last_slices, self.buf = (0, []), [], None
        self.cap, self.payloads = 64, {}


class WH:
    """routes=None: an echo (streams = the source's, which are the outgoing ones too); routes = {from: to}: a proxy, the
    replies go out on a transport of their own that holds out_streams"""

    def __init__(self, g, streams=(1, 3, 5), routes=None, out_streams=(), arena_bytes=1 << 16, max_frame=16384,
                 max_pending=4096, max_messages=4096, initial_window=65535, conn_window=65535, peer_max_frame=16384,
                 max_msg=4 << 20, asm_pending=4096, table_slots=0, cap=256, attach=True):
        from grpc_rdma_amd import h2dev
        self.g, self.h2dev, self.cap = g, h2dev, cap
        self.r = RHarness(g, arena_bytes, max_msg, asm_pending, streams=streams, table_slots=table_slots)
        if routes is None:
            self.s = SHOn(g, self.r.pp, streams, initial_window, conn_window, peer_max_frame)
        else:
            self.s = SH(g, streams=out_streams, initial_window=initial_window, conn_window=conn_window,
                        peer_max_frame=peer_max_frame, table_slots=table_slots)
            self.s.named |= set(routes.values())
        self.echo = routes is None
        self.reply = h2dev.Reply(self.r.asm, sorted(routes.items()) if routes else None, max_frame, max_messages)
        if attach:
            self.reply.attach_windows(self.s.sw, max_pending)
        self.model = WindowedReplyModel(self.r.model, self.s.model, max_frame, routes, max_pending, max_messages)
        self.releasable = 0

    # ---- the receiving side ----------------------------------------------------------------------------------------
    def receive(self, slices):
        """one grdma_h2_deframe_messages call of the source (device and models, compared); an echo's send windows
        take the same call in"""
        got, _, ev_o = self.r.feed(slices, want_events=True)
        self.model.source_call(self.r.last)
        if self.echo:
            self.s.last, self.s.last_slices = (self.r.pp.err, ev_o), slices
            self.s.intake()
        return got

    def skipped_receive(self, slices, ev_cap):
        """a source call whose event list overflows: the assembler skips it and reports nothing (a proxy's source: an
        echo's send windows would have to take the same lost call in)"""
        same(self.echo, False, "skipped_receive is for a proxy's source")
        buf, table = self.r.pp.upload(slices)
        self.r.pp.expect(slices)
        with pytest.raises(self.g.GrdmaError, match="error 5"):
            self.r.parser.deframe_messages(buf.ptr, table, self.r.asm, ev_cap=ev_cap)
        self.r.last = []
        self.model.source_call([], skipped=True)

    def credit(self, slices):
        """control frames for the outgoing transport through a PLAIN deframing and the intake (no source call)"""
        return self.s.feed(slices)

    def release(self, n=None):
        n = self.releasable if n is None else n
        self.r.asm.release(n)
        self.r.model.release(n)
        self.releasable = 0
        self.check_ring()

    def check_ring(self):
        same(self.r.asm.stats()["bytes_in_use"], self.r.model.bytes_in_use(), "assembler: bytes in use")

    # ---- the sending side --------------------------------------------------------------------------------------------
    def new_target(self, cap):
        self.slices = self.g.DeviceBuffer(data=bytes([SENTINEL]) * (16 * (cap + 4)))
        self.hdr = self.g.DeviceBuffer(data=bytes([SENTINEL]) * (32 * (cap + 4)))

    def wire_of(self, sl, hdr):
        """the bytes the slice list names: inlined slices from the header arena, the others from the assembler's ring"""
        arena, out = self.r.arena.read(), bytearray()
        for ptr, n in sl:
            if self.hdr.ptr <= ptr and ptr + n <= self.hdr.ptr + len(hdr):
                out += hdr[ptr - self.hdr.ptr:ptr - self.hdr.ptr + n]
            elif self.r.arena.ptr <= ptr and ptr + n <= self.r.arena.ptr + len(arena):
                out += arena[ptr - self.r.arena.ptr:ptr - self.r.arena.ptr + n]
            else:
                raise AssertionError("a slice (%#x, %d) outside the header arena and the assembler's ring" % (ptr, n))
        return bytes(out)

    def check_written(self, sl, res, what):
        """the slice table and the header arena as a whole: what the call wrote, the fill everywhere else -> the wire"""
        raw = self.slices.read()
        same(read_slices(self.g, self.slices, len(sl)), sl, what + ": slice table")
        same(raw[16 * len(sl):], bytes([SENTINEL]) * (len(raw) - 16 * len(sl)), what + ": slice table behind the slices")
        hdr = self.hdr.read()
        inl = [p for p, n in sl if self.hdr.ptr <= p < self.hdr.ptr + self.hdr.nbytes]
        same(inl, [self.hdr.ptr + 32 * k for k in range(len(inl))], what + ": inlined slice pointers")
        same(32 * len(inl), res[3], what + ": header-arena bytes")
        same(hdr[32 * len(inl):], bytes([SENTINEL]) * (len(hdr) - 32 * len(inl)), what + ": header arena behind the slices")
        return self.wire_of(sl, hdr)

    def expect(self, cap=None, hdr_cap=None, pending_only=False):
        """the model's side of one call and a fresh target -> the item (Reply, slices, cap, header arena, cap, flag) of
        h2dev.reply_frame_windowed_batch; `check` compares what the device made of it"""
        cap = self.cap if cap is None else cap
        hdr_cap = 32 * cap if hdr_cap is None else hdr_cap
        self.new_target(max(cap, 1))
        self.expected = self.model.frame(self.s.live(), cap, hdr_cap, pending_only)
        return (self.reply, self.slices.ptr, cap, self.hdr.ptr, hdr_cap, pending_only)

    def check(self, sl, st, what="windowed reply"):
        """sl: the device's slice list, None where the call overflowed; st: its result dict -> (wire, result tuple)"""
        lens, wire, res = self.expected
        got = tuple(st[k] for k in WORDS)
        print("%s: %r -> %r" % (what, res, got))
        same(got, res, what + ": result")
        same(st["spare"], 0, what + ": spare word")
        if res[7]:
            same(sl, None, what + ": what an overflowing call hands back")
            same(self.slices.read(), bytes([SENTINEL]) * self.slices.nbytes, what + ": slice table of an overflowing call")
            same(self.hdr.read(), bytes([SENTINEL]) * self.hdr.nbytes, what + ": header arena of an overflowing call")
        else:
            same([n for _, n in sl], lens, what + ": slice lengths")
            same(self.check_written(sl, res, what), wire, what + ": wire")
            self.last_slices = sl
        same(self.reply.pending(), self.model.pending(), what + ": the queue (stream, length, progress)")
        self.s.check()
        self.check_ring()
        self.releasable = res[12]
        return wire, res

    def frame(self, cap=None, hdr_cap=None, pending_only=False, what="windowed reply"):
        """one call on the device and in the model, compared -> (wire, result tuple in the order of WORDS)"""
        item = self.expect(cap, hdr_cap, pending_only)
        if self.expected[2][7]:
            with pytest.raises(self.g.GrdmaError, match="error 5"):
                self.reply.frame_windowed(*item[1:])
            return self.check(None, self.reply.last_windowed, what)
        sl, st = self.reply.frame_windowed(*item[1:])
        return self.check(sl, st, what)

    def close(self):
        self.reply.close()
        self.s.sw.close()
        self.r.close()
        if not self.echo:
            self.s.parser.close()


def frame_batch(hs, kw=None):
    """one h2dev.reply_frame_windowed_batch over the harnesses hs, in that order (kw: per harness the arguments of
    WH.expect); every item is compared with its own model as a single call is -> [(wire, result tuple)]"""
    from grpc_rdma_amd import h2dev
    kw = kw or [{}] * len(hs)
    items = [h.expect(**k) for h, k in zip(hs, kw)]
    got = h2dev.reply_frame_windowed_batch(items)
    out = []
    for i, (h, (sl, st)) in enumerate(zip(hs, got)):
        same(sl == -5, bool(h.expected[2][7]), "item %d: -GRDMA_ERR_CAPACITY where the model overflows" % i)
        out.append(h.check(None if sl == -5 else sl, st, "batch item %d" % i))
    return out
