"""The harness of the send flow control device tests (tests/test_zz_gpu_h2_send_window.py): a device parser with its send
windows (h2dev.SendWindows), the oracle's parser and the model of tests/h2_send_model.py beside them.  Every call runs on
the device and in the model and is compared exactly: result blocks, windows, counters, progress, slice lists, wire images.
pytest rewrites no `assert` in a helper module, so every check here goes through `same`."""
import struct

import pytest

from tests.h2_device_lib import SENTINEL, ParserPair, read_slices, same
from tests.h2_helpers import frame
from tests.h2_send_model import SendModel, live_of


def window_update(sid, inc):
    return frame(8, 0, sid, struct.pack(">I", inc))


def settings(entries, ack=False):
    return frame(4, 1 if ack else 0, 0, b"".join(struct.pack(">HI", i, v) for i, v in entries))


def body(n, seed=0):
    return bytes((j * 7 + seed * 13 + 1) % 251 for j in range(n))


class SH:
    def __init__(self, g, prefix=False, streams=(), initial_window=65535, conn_window=65535, peer_max_frame=16384,
                 table_slots=0, cap=64):
        from grpc_rdma_amd import h2dev
        self.g, self.h2dev = g, h2dev
        orc_kw = dict(max_concurrent_streams=table_slots // 2) if table_slots else None
        self.pp = ParserPair(g, prefix, streams, orc_kw=orc_kw, table_slots=table_slots)
        self.parser = self.pp.dev
        self.sw = h2dev.SendWindows(self.parser, initial_window, conn_window, peer_max_frame)
        self.model = SendModel(initial_window, conn_window, peer_max_frame)
        self.named = set(streams)
        self.last, self.last_slices, self.buf = (0, []), [], None
        self.cap = cap
        self.payloads = {}

    # ---- the receiving side ----------------------------------------------------------------------------------------
    def live(self):
        return live_of(self.pp.orc)

    def deframe(self, slices, ev_cap=None, checked=True):
        """one standalone deframing on the device and in the oracle; the arena stays until the next one"""
        self.buf, table = self.pp.upload(slices)
        self.last, self.last_slices = self.pp.expect(slices), slices
        got = self.parser.deframe(self.buf.ptr, table, cap=ev_cap or 8 * len(slices) + 4096)
        if checked:
            same(got[0], self.last[0], "h2 error")
            same(got[1], self.last[1], "events")
        return got

    def intake(self):
        """take the last deframing in on the device and in the model, compare -> the result"""
        err_o, ev_o = self.last
        res = self.model.intake(ev_o, self.last_slices, err_o, self.live())
        got = self.sw.intake()
        print("intake: %r -> %r" % (res, got))
        same(got, res, "intake: result")
        self.check()
        return res

    def feed(self, slices, ev_cap=None):
        self.deframe(slices, ev_cap)
        return self.intake()

    def check(self):
        ids = [0] + sorted(self.named - {0})
        same(self.sw.windows(ids), [self.model.window(i) for i in ids], "windows of %r" % (ids,))
        st = self.sw.stats()
        same({k: st[k] for k in self.model.stats}, self.model.stats, "counters (all: %r)" % (st,))
        same((st["lost"], st["initial_window"], st["max_frame"]), (self.model.lost, self.model.iws, self.model.pmf),
             "(lost, the peer's INITIAL_WINDOW_SIZE, MAX_FRAME_SIZE)")

    # ---- the sending side --------------------------------------------------------------------------------------------
    def upload_bodies(self, msgs):
        """msgs: [(body, stream, flags)] -> the device table [(ptr, len, stream, flags)]; bodies share one arena"""
        arena, offs = bytearray(), []
        for b, _, _ in msgs:
            offs.append(len(arena))
            arena += b + bytes((-len(b)) % 16)
        self.pay_host = bytes(arena) + bytes(16)
        self.pay = self.g.DeviceBuffer(data=self.pay_host)
        return [(self.pay.ptr + o, len(b), s, f) for o, (b, s, f) in zip(offs, msgs)]

    def new_target(self, cap):
        self.slices = self.g.DeviceBuffer(data=bytes([SENTINEL]) * (16 * (cap + 4)))
        self.hdr = self.g.DeviceBuffer(data=bytes([SENTINEL]) * (32 * (cap + 4)))

    def wire_of(self, sl):
        """the bytes the slice list names, read from the header arena and the payload arena (one copy each)"""
        hdr, out = self.hdr.read(), bytearray()
        for ptr, n in sl:
            if self.hdr.ptr <= ptr and ptr + n <= self.hdr.ptr + len(hdr):
                out += hdr[ptr - self.hdr.ptr:ptr - self.hdr.ptr + n]
            elif self.pay.ptr <= ptr and ptr + n <= self.pay.ptr + len(self.pay_host):
                out += self.pay_host[ptr - self.pay.ptr:ptr - self.pay.ptr + n]
            else:
                raise AssertionError("a slice (%#x, %d) outside the header arena and the payloads" % (ptr, n))
        return bytes(out)

    def frame(self, msgs, progress, max_frame, cap=None, hdr_cap=None, table=None):
        """one framing call on the device and in the model, compared -> (wire, result, progress after the call)"""
        cap = self.cap if cap is None else cap
        hdr_cap = 32 * cap if hdr_cap is None else hdr_cap
        self.named |= {s for _, s, _ in msgs}
        table = table or self.upload_bodies(msgs)
        self.new_target(max(cap, 1))
        lens, wire, res, prog = self.model.frame(msgs, progress, max_frame, cap, hdr_cap, self.live())
        if res[7]:
            with pytest.raises(self.g.GrdmaError, match="error 5"):
                self.sw.frame(table, progress, max_frame, self.slices.ptr, cap, self.hdr.ptr, hdr_cap)
            same(self.sw.last_result, res, "frame: result of an overflowing call")
            same(self.slices.read(), bytes([SENTINEL]) * self.slices.nbytes, "frame: slice table of an overflowing call")
            same(self.hdr.read(), bytes([SENTINEL]) * self.hdr.nbytes, "frame: header arena of an overflowing call")
        else:
            sl, got, prog_d = self.sw.frame(table, progress, max_frame, self.slices.ptr, cap, self.hdr.ptr, hdr_cap)
            print("frame: %r -> %r" % (res, got))
            same(got, res, "frame: result")
            same(prog_d, prog, "frame: progress")
            same([n for _, n in sl], lens, "frame: slice lengths")
            same(read_slices(self.g, self.slices, len(sl)), sl, "frame: slice table")
            same(self.wire_of(sl), wire, "frame: wire")
            # inlined slices lie in the header arena, 32 bytes apart, in slice order
            inl = [p for p, n in sl if self.hdr.ptr <= p < self.hdr.ptr + self.hdr.nbytes]
            same(inl, [self.hdr.ptr + 32 * k for k in range(len(inl))], "frame: inlined slice pointers")
            same(32 * len(inl), res[3], "frame: header-arena bytes")
        self.check()
        self.last_frame = (lens, wire, res, prog)
        return wire, res, prog

    def close(self):
        self.sw.close()
        self.parser.close()
