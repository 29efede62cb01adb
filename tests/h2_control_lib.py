"""The harness of the control-reply device tests (tests/test_zz_gpu_h2_control.py, tests/test_zz_gpu_h2_links_control.py): a
device parser with its control-reply writer (h2dev.ControlReplies), the oracle's parser and the model of
tests/h2_control_model.py beside them.  Every call runs on the device and in the model and is compared exactly: slices,
the whole slice table and header arena (what the call must not touch keeps its fill), result block, peer record, counters.
pytest rewrites no `assert` in a helper module, so every check here goes through `same`."""
import pytest

from tests.h2_control_model import PEER_KEYS, STAT_KEYS, ControlModel
from tests.h2_device_lib import SENTINEL, ParserPair, read_slices, same
from tests.h2_helpers import frame, grpc_msg

ERR5 = "error 5"  # -GRDMA_ERR_CAPACITY


def settings(n=1, ack=False):
    return frame(4, 1 if ack else 0, 0, b"" if ack else b"".join((3).to_bytes(2, "big") + (100 + k).to_bytes(4, "big") for k in range(n)))


def ping(opaque, ack=False):
    opaque = opaque.to_bytes(8, "big") if isinstance(opaque, int) else opaque
    return frame(6, 1 if ack else 0, 0, opaque)


def goaway(last_stream, code, debug=b""):
    return frame(7, 0, 0, last_stream.to_bytes(4, "big") + code.to_bytes(4, "big") + debug)


def data(sid, body=b"abc", flags=0):
    return frame(0, flags, sid, grpc_msg(body))


def bad_flags(sid, n=3):
    return frame(0, 2, sid, bytes(n))  # (a DATA flag that is none: a stream error in the frame header)


def bad_grpc(sid, good=1, tail=4):
    """a DATA frame whose payload holds `good` messages and then a byte that is no gRPC flag"""
    return frame(0, 0, sid, grpc_msg(b"ok") * good + b"\x07" + bytes(tail))


def cut_at(wire, *points):
    pts = (0,) + tuple(points) + (len(wire),)
    return [wire[a:b] for a, b in zip(pts, pts[1:]) if b > a]


def expected_arena(wire, lens, nbytes):
    """the header arena behind a call: slice k's bytes at 32 k, everything else as it was"""
    exp = bytearray([SENTINEL]) * nbytes
    for k, n in enumerate(lens):
        exp[32 * k:32 * k + n] = wire[23 * k:23 * k + n]
    return bytes(exp)


class Target:
    """a slice table and a header arena filled with SENTINEL, with room for `cap` slices"""

    def __init__(self, g, cap):
        self.cap = cap
        self.slices = g.DeviceBuffer(data=bytes([SENTINEL]) * (16 * (cap + 4)))
        self.hdr = g.DeviceBuffer(data=bytes([SENTINEL]) * (32 * (cap + 4)))

    def check(self, g, sl, lens, wire, what):
        """the device's slice list `sl` and the memory behind it against the model's lens / wire"""
        same([n for _, n in sl], lens, what + ": slice lengths")
        same([p for p, _ in sl], [self.hdr.ptr + 32 * k for k in range(len(lens))], what + ": slice pointers")
        raw = self.slices.read()
        same(read_slices(g, self.slices, len(sl)), sl, what + ": slice table")
        same(raw[16 * len(sl):], bytes([SENTINEL]) * (len(raw) - 16 * len(sl)), what + ": slice table behind the list")
        same(self.hdr.read(), expected_arena(wire, lens, self.hdr.nbytes), what + ": header arena")

    def untouched(self, what):
        same(self.slices.read(), bytes([SENTINEL]) * self.slices.nbytes, what + ": slice table untouched")
        same(self.hdr.read(), bytes([SENTINEL]) * self.hdr.nbytes, what + ": header arena untouched")


class CH:
    def __init__(self, g, prefix=False, streams=(), max_replies=4096, cap=64):
        from grpc_rdma_amd import h2dev
        self.g, self.h2dev = g, h2dev
        self.pp = ParserPair(g, prefix, streams)
        self.parser = self.pp.dev
        self.ctl = h2dev.ControlReplies(self.parser, max_replies)
        self.model = ControlModel(max_replies)
        self.last, self.last_slices, self.buf = (0, []), [], None
        self.cap = cap
        self.skipped = False

    def deframe(self, slices, ev_cap=None, checked=True):
        """one standalone deframing on the device and in the oracle; the arena stays until the next one"""
        self.buf, table = self.pp.upload(slices)
        self.last, self.last_slices = self.pp.expect(slices), slices
        got = self.parser.deframe(self.buf.ptr, table, cap=ev_cap or 8 * len(slices) + 4096)
        if checked:
            same(got[0], self.last[0], "h2 error")
            same(got[1], self.last[1], "events")
        return got

    def expect(self, cap, hdr_cap):
        err_o, ev_o = self.last
        exp = self.model.reply(ev_o, self.last_slices, err_o, cap, hdr_cap, self.skipped)
        if exp[2][7] != 1:
            self.skipped = False
        return exp

    def reply(self, cap=None, hdr_cap=None):
        """answer the last deframing on the device and in the model, compare -> (wire, result)"""
        cap = self.cap if cap is None else cap
        hdr_cap = 32 * cap if hdr_cap is None else hdr_cap
        t = self.target = Target(self.g, max(cap, 1))
        lens, wire, res = self.expect(cap, hdr_cap)
        if res[7]:
            with pytest.raises(self.g.GrdmaError, match=ERR5):
                self.ctl.reply(t.slices.ptr, cap, t.hdr.ptr, hdr_cap)
            same(self.ctl.last_result, res, "reply: result of an overflowing call")
            t.untouched("an overflowing call")
        else:
            sl, got = self.ctl.reply(t.slices.ptr, cap, t.hdr.ptr, hdr_cap)
            print("reply: %r -> %r" % (res, got))
            same(got, res, "reply: result")
            t.check(self.g, sl, lens, wire, "reply")
        self.check()
        return wire, res

    def feed(self, slices, ev_cap=None, **kw):
        self.deframe(slices, ev_cap)
        return self.reply(**kw)

    def check(self):
        peer = self.ctl.peer()
        same({k: peer[k] for k in PEER_KEYS}, self.model.peer, "what the peer said")
        st = self.ctl.stats()
        same({k: st[k] for k in STAT_KEYS}, self.model.stats, "counters (all: %r)" % (st,))
        same(st["lost"], self.model.lost, "the sticky flag")

    def close(self):
        self.ctl.close()
        self.parser.close()


# ---- many links: a list of CH under the batch call ---------------------------------------------------------------------
def reply_batch(hs, order, caps=None, lost=()):
    """one h2dev.control_batch over the links listed in `order`, every item against its own link's model -> {link:
    (wire, result)}.  caps: {link: (slices cap, header cap)} where they differ from the link's; lost: links whose last
    deframing overflowed its event list"""
    h2dev = hs[order[0]].h2dev
    items, exp = [], {}
    for i in order:
        h = hs[i]
        cap, hdr_cap = (caps or {}).get(i, (h.cap, 32 * h.cap))
        h.target = Target(h.g, max(cap, 1))
        exp[i] = h.model.lost_call() if i in lost else h.expect(cap, hdr_cap)
        items.append((h.ctl, h.target.slices.ptr, cap, h.target.hdr.ptr, hdr_cap))
    got = h2dev.control_batch(items)
    same(len(got), len(order), "control_batch: items")
    out = {}
    for k, i in enumerate(order):
        h = hs[i]
        lens, wire, res = exp[i]
        what = "link %d reply" % i
        print("%s: %r -> %r" % (what, res, got[k][0] if res[7] else got[k][1]))
        if res[7]:
            same(got[k], (res, None), what + ": what an overflowing item hands back")
            h.target.untouched(what + " (overflow)")
        else:
            same(got[k][1], res, what + ": result")
            h.target.check(h.g, got[k][0], lens, wire, what)
        same(h.ctl.last_result, res, what + ": .last_result")
        h.check()
        out[i] = (wire, res)
    return out


def reply_batch_raw(hs, order, caps=None):
    """grdma_h2_ctl_reply_batch itself, into fresh targets -> (its return value, the result tuples)"""
    import ctypes as C
    h2dev = hs[order[0]].h2dev
    arr = (h2dev.H2CtlItem * len(order))()
    for k, i in enumerate(order):
        h = hs[i]
        cap, hdr_cap = (caps or {}).get(i, (h.cap, 32 * h.cap))
        h.target = Target(h.g, max(cap, 1))
        arr[k].ctl = h.ctl.h
        arr[k].d_slices_out, arr[k].slices_cap, arr[k].d_hdr_arena, arr[k].hdr_cap = h.target.slices.ptr, cap, h.target.hdr.ptr, hdr_cap
    out = (C.c_uint64 * (8 * len(order)))()
    rc = h2dev.load().grdma_h2_ctl_reply_batch(arr, len(order), out)
    return rc, [tuple(int(x) for x in out[8 * k:8 * k + 8]) for k in range(len(order))]
