"""The harness of the HTTP/2 device tests (tests/test_gpu_h2.py, tests/test_zz_gpu_h2_*.py) and what the CPU-side
HTTP/2 tests share with them.  A test file imports from here, from tests/h2_helpers.py (byte builders),
tests/h2_asm_model.py (the assembler's model), tests/h2_flow_model.py (the ledger's model), from `oracle` and from the
package -- never from another test file.

docs/h2_deframer.md ("Writing a test for an HTTP/2 kernel") lists what is here.  pytest rewrites no `assert` in a helper
module, so every check in this file goes through `same` or carries its values in its message.  The wire generators are
seeded and feed exact comparisons: tests/test_h2_device_lib.py pins their outputs and the packer's layouts.

A new HTTP/2 device test file: build wires with h2_helpers and the generators here, run them through a ParserPair (or
Harness / FH where an assembler or ledger is under test), compare with `same`, and keep only what is its own."""
import ctypes as C
import json
import os
import random

import pytest

from oracle import pyorc
from tests.h2_asm_model import OK, AsmModel
from tests.h2_flow_model import Model
from tests.h2_helpers import PREFACE, frame, grpc_msg

SENTINEL = 0xA5
ERR_INVALID, ERR_CAPACITY = 2, 5  # GRDMA_ERR_INVALID, GRDMA_ERR_CAPACITY: a call returns the negative
VEC = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "h2_bad_client.json")))["vectors"]


# ---- comparisons -----------------------------------------------------------------------------------------------------
def _show(v):
    r = v.hex() if isinstance(v, (bytes, bytearray)) else repr(v)
    return r if len(r) <= 400 else r[:400] + "..."


def same(got, exp, what=""):
    """got == exp, or an AssertionError that says where: for two sequences the index of the first difference, both
    lengths and the two items there (bytes: the 16 bytes from there on)"""
    if got == exp:
        return
    seq = (list, tuple, bytes, bytearray)
    if isinstance(got, seq) and isinstance(exp, seq):
        n = min(len(got), len(exp))
        bad = next((i for i in range(n) if got[i] != exp[i]), n)
        w = 16 if isinstance(got, (bytes, bytearray)) else 1
        raise AssertionError("%s: item %d of %d / %d: device %s, expected %s" % (
            what, bad, len(got), len(exp), _show(got[bad:bad + w]), _show(exp[bad:bad + w])))
    raise AssertionError("%s: device %s, expected %s" % (what, _show(got), _show(exp)))


# ---- byte movers -----------------------------------------------------------------------------------------------------
def read_slices(g, slices_buf, n):
    raw = slices_buf.read(16 * n)
    out = []
    for i in range(n):
        ptr = int.from_bytes(raw[16 * i:16 * i + 8], "little")
        ln = int.from_bytes(raw[16 * i + 8:16 * i + 16], "little")
        out.append((ptr, ln))
    return out


def device_bytes(g, ptr, n):
    dst = C.create_string_buffer(max(1, n))
    if n:
        g._lib.check(g.load().grdma_copy_to_host(dst, ptr, n))
    return dst.raw[:n]


PADDED, UNPADDED, STEPPED = "padded", "unpadded", "stepped"


def pack_slices(slices, layout=PADDED, rng=None):
    """The slices in one arena -> (arena bytes, [(offset, len)]); 64 zero bytes behind the last slice.
    PADDED: every slice is followed by zeros up to a multiple of 16 of its own length.  UNPADDED: nothing behind a
    slice; without a generator every slice starts on a multiple of 16.  In both a generator puts 1..15 bytes of 0xEE in
    front of every slice (one randrange(1, 16) per slice), so the offsets are odd.  STEPPED: 1 + 5 k mod 15 bytes of
    0xEE in front of slice k, no generator."""
    arena, table = bytearray(), []
    for k, s in enumerate(slices):
        if layout == STEPPED:
            arena += b"\xee" * (1 + (5 * k) % 15)
        elif rng is not None:
            arena += b"\xee" * rng.randrange(1, 16)
        elif layout == UNPADDED:
            arena += bytes((-len(arena)) % 16)
        table.append((len(arena), len(s)))
        arena += s
        if layout == PADDED:
            arena += bytes((-len(s)) % 16)
    return bytes(arena) + bytes(64), table


# ---- the oracle over one call ----------------------------------------------------------------------------------------
def oracle_parser(prefix, max_frame=16384, streams=(), **kw):
    p = pyorc.H2Parser(expect_client_prefix=prefix, max_frame_size=max_frame, **kw)
    for sid in streams:
        rc = p.open_stream(sid)
        assert rc == 0, "oracle open_stream(%d) = %d" % (sid, rc)
    return p


def oracle_feed(parser, slices, cap=None):
    """-> (h2 error, events tagged with the slice index); stops at the first error.  cap: the event cap of every feed,
    a number or a function of the slice (None: pyorc's default of two events per byte)"""
    out = []
    for i, s in enumerate(slices):
        rc, ev = parser.feed(s, cap=cap(s) if callable(cap) else cap)
        out += [(k, a, b, c, d, i) for k, a, b, c, d in ev]
        if rc:
            return rc, out
    return 0, out


def oracle_events(slices, prefix, max_frame=16384, streams=(), cap=None):
    return oracle_feed(oracle_parser(prefix, max_frame, streams), slices, cap)


# ---- one transport: a device parser and the oracle's beside it -------------------------------------------------------
class ParserPair:
    """A device h2dev.Parser and the oracle's pyorc.H2Parser with the same streams.  expect() is the oracle over one
    call, upload() puts a call's slices into device memory, call() runs one deframe call on both and compares."""
    layout = PADDED
    orc_cap = None   # the oracle's event cap per slice (see oracle_feed)

    def __init__(self, g, prefix, streams=(), max_frame=16384, orc_kw=None, **dev_kw):
        from grpc_rdma_amd import h2dev
        self.g = g
        self.dev = h2dev.Parser(prefix, max_frame, **dev_kw)
        self.orc = pyorc.H2Parser(expect_client_prefix=prefix, max_frame_size=max_frame, **(orc_kw or {}))
        self.err, self.ncalls = 0, 0
        if streams:
            self.open(streams)

    def open(self, ids):
        same(self.dev.open_streams(ids), 0, "open_streams")
        for s in ids:
            same(self.orc.open_stream(s), 0, "oracle open_stream(%d)" % s)

    def close_writes(self, ids):
        same(self.dev.close_writes(ids), 0, "close_writes")
        for s in ids:
            same(self.orc.close_writes(s), 0, "oracle close_writes(%d)" % s)

    def live(self):
        n = self.dev.live_streams()
        same(n, self.orc.live_streams(), "live streams after call %d" % self.ncalls)
        return n

    def expect(self, slices):
        """the oracle over one call -> (h2 error, events); behind a connection error every call is (that error, [])"""
        if self.err:
            return self.err, []
        self.err, ev = oracle_feed(self.orc, slices, self.orc_cap)
        return self.err, ev

    def upload(self, slices, rng=None):
        """-> (DeviceBuffer, slice table) of one call over `slices`, which go into an arena of their own"""
        data, table = pack_slices(slices, self.layout, rng)
        return self.g.DeviceBuffer(data=data), table

    def call(self, slices, rng=None, want_err=0, cap=None):
        """one deframe call on both -> the events"""
        buf, table = self.upload(slices, rng)
        err, ev = self.dev.deframe(buf.ptr, table, cap=cap or 8 * len(slices) + 4096)
        buf.free()
        err_o, ev_o = self.expect(slices)
        self.ncalls += 1
        same((err, err_o), (want_err, want_err), "call %d: h2 error (device, oracle)" % self.ncalls)
        same(ev, ev_o, "call %d events" % self.ncalls)
        return ev

    def close(self):
        self.dev.close()


class Transport(ParserPair):
    """one connection with the slices still to be delivered; item() is its entry in a batch call"""

    def __init__(self, g, name, prefix, slices, streams=(), max_frame=16384):
        ParserPair.__init__(self, g, prefix, streams, max_frame)
        self.name, self.slices, self.bufs = name, list(slices), []

    def item(self, slices, rng=None):
        """(parser, arena ptr, slice table) of one call over `slices`"""
        buf, table = self.upload(slices, rng)
        self.bufs.append(buf)
        return (self.dev, buf.ptr, table)


class Both(ParserPair):
    """The same calls on a device parser with the boundary step and on the oracle's; no call may fail."""
    layout, orc_cap = UNPADDED, 1024

    def __init__(self, g, prefix, streams=(), chunks=None, gap_seed=None):
        ParserPair.__init__(self, g, prefix, streams, boundary_step=True, chunks=chunks)
        self.rng = random.Random(gap_seed) if gap_seed is not None else None

    def call(self, slices):
        return len(ParserPair.call(self, slices, self.rng))


class Conn(ParserPair):
    """a device parser with a small stream map: every call's events and the number of live streams equal the oracle's;
    the messages are rebuilt from the DEVICE's events"""

    def __init__(self, g, prefix, slots=16, **kw):
        ParserPair.__init__(self, g, prefix, orc_kw=dict(max_concurrent_streams=slots // 2), table_slots=slots, **kw)
        self.partial, self.done = {}, []

    def open(self, ids):
        ParserPair.open(self, ids)
        self.live()

    def close_writes(self, ids):
        ParserPair.close_writes(self, ids)
        self.live()

    def call(self, slices, want_err=0, cap=None):
        ev = ParserPair.call(self, slices, want_err=want_err, cap=cap)
        self.live()
        for k, a, b, c, d, i in ev:
            if k == 3:
                self.partial[c] = bytearray()
            elif k == 4:
                self.partial[c] += slices[i][a:a + b]
            elif k == 5:
                self.done.append((c, bytes(self.partial.pop(c))))
            elif k == 7:
                self.partial.pop(c, None)
        return ev


# ---- the assembler and the ledger beside a ParserPair ----------------------------------------------------------------
class Harness:
    """one device parser + assembler, the oracle's parser and the model beside them; feed() runs one call on both and
    checks it"""

    def __init__(self, g, arena_bytes, max_msg=4 << 20, max_pending=4096, prefix=False, streams=(), max_frame=16384,
                 chunks=None, tensor=None, table_slots=0):
        from grpc_rdma_amd import h2dev
        self.g, self.h2dev = g, h2dev
        self.pp = ParserPair(g, prefix, streams, max_frame, chunks=chunks, table_slots=table_slots)
        self.parser = self.pp.dev
        self.arena = tensor if tensor is not None else g.DeviceBuffer(data=bytes([SENTINEL]) * arena_bytes)
        self.asm = h2dev.Assembler(self.parser, self.arena, max_msg, max_pending)
        self.model = AsmModel(arena_bytes, max_msg, max_pending)

    def expect(self, slices):
        """the oracle's parser, then the model over its events -> (h2 error, events, [(descriptor, bytes)])"""
        err_o, ev_o = self.pp.expect(slices)
        return err_o, ev_o, self.model.call(ev_o, slices, err_o)

    def feed(self, slices, rng=None, want_events=False):
        buf, table = self.pp.upload(slices, rng)
        r = self.parser.deframe_messages(buf.ptr, table, self.asm, want_events=want_events)
        err_o, ev_o, exp = self.expect(slices)
        err, got = r[0], r[1]
        same(err != 0, err_o != 0, "h2 error %d, the oracle's %d" % (err, err_o))
        same([tuple(m) for m in got], [d for d, _ in exp], "descriptors")
        for m, (_, body) in zip(got, exp):
            if m.status == OK:
                v = self.asm.view(m)
                v = bytes(v.cpu().numpy().tobytes()) if hasattr(v, "cpu") else v
                same(v, body, "message seq %d" % m.seq)
        if want_events:
            return got, r[2], ev_o
        return got

    def release(self, n=None):
        self.asm.release(n if n is not None else (1 << 63))
        self.model.release(n)

    def close(self):
        self.asm.close()
        self.parser.close()


class RHarness(Harness):
    """Harness that keeps what the model reported for the last call: [((offset, length, seq, stream, status, flags),
    body or None)]"""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.last = []
        call = self.model.call

        def keeping(events, slices, h2_error=0):
            self.last = call(events, slices, h2_error)
            return self.last

        self.model.call = keeping


class FH:
    """a device parser with its ledger, the oracle's parser and the model beside them"""

    def __init__(self, g, prefix=False, streams=(), stream_window=65535, conn_window=65535, conn_threshold=0,
                 max_updates=64, cap=None, chunks=None, boundary_step=None, table_slots=0):
        from grpc_rdma_amd import h2dev
        self.g, self.h2dev = g, h2dev
        self.pp = ParserPair(g, prefix, streams, chunks=chunks, boundary_step=boundary_step, table_slots=table_slots)
        self.parser = self.pp.dev
        self.fc = h2dev.FlowControl(self.parser, stream_window=stream_window, conn_window=conn_window,
                                    conn_threshold=conn_threshold, max_updates=max_updates)
        self.model = Model(stream_window, conn_window, conn_threshold, max_updates, streams)
        self.cap = cap if cap is not None else (13 * max_updates + 22) // 23
        self.last = (0, [])
        self.new_target()

    def new_target(self):
        self.slices = self.g.DeviceBuffer(data=bytes([SENTINEL]) * (16 * (self.cap + 4)))
        self.hdr = self.g.DeviceBuffer(data=bytes([SENTINEL]) * (32 * (self.cap + 4)))

    def told(self, slices):
        """the oracle takes a call (one the device parser was given elsewhere, or is given next)"""
        self.last = self.pp.expect(slices)

    def deframe(self, slices, ev_cap=None):
        self.buf, table = self.pp.upload(slices)
        self.told(slices)
        return self.parser.deframe(self.buf.ptr, table, cap=ev_cap or 8 * len(slices) + 4096)

    def oracle(self):
        """(h2 error, events) of the oracle for the last call"""
        return self.last

    def account(self, cap=None, hdr_cap=None):
        """account the last deframing on the device and in the model, compare, -> (result, wire)"""
        cap = self.cap if cap is None else cap
        hdr_cap = 32 * cap if hdr_cap is None else hdr_cap
        err_o, ev_o = self.oracle()
        lens, res, wire = self.model.call(ev_o, err_o, cap, hdr_cap)
        if res[7]:
            with pytest.raises(self.g.GrdmaError, match="error 5"):
                self.fc.account(self.slices.ptr, cap, self.hdr.ptr, hdr_cap)
            got = None
        else:
            got = self.fc.account(self.slices.ptr, cap, self.hdr.ptr, hdr_cap)
            print("ledger: %r -> %r" % (res, got[1]))
        self.check_accounted((lens, res, wire), got)
        return res, wire

    def check_accounted(self, exp, got, what="ledger"):
        """exp = the model's (slice lengths, result, wire) of a call; got = the device's (slices, result, wire), None
        where the call overflowed: then the result block is there and nothing was written"""
        lens, res, wire = exp
        if res[7]:
            same(got, None, what + ": what an overflowing call hands back")
            same(self.fc.last_result, res, what + ": result of an overflowing call")
            same(self.slices.read(), bytes([SENTINEL]) * self.slices.nbytes, what + ": slice table of an overflowing call")
            same(self.hdr.read(), bytes([SENTINEL]) * self.hdr.nbytes, what + ": header arena of an overflowing call")
        else:
            sl, r, w = got
            same(r, res, what + ": result")
            same([n for _, n in sl], lens, what + ": slice lengths")
            same([p for p, _ in sl], [self.hdr.ptr + 32 * k for k in range(len(sl))], what + ": slice pointers")
            same(w, wire, what + ": wire")
            same(read_slices(self.g, self.slices, len(sl)), sl, what + ": slice table")
        self.check_stats()

    def check_stats(self):
        st = self.fc.stats()
        same({k: st[k] for k in self.model.stats}, self.model.stats, "ledger counters (all: %r)" % (st,))
        same((st["announced"], st["lost"]), (self.model.announced, self.model.lost), "ledger (announced, lost)")

    def deframe_checked(self, slices, ev_cap=None):
        got = self.deframe(slices, ev_cap)
        same(got[0], self.oracle()[0], "h2 error")
        same(got[1], self.oracle()[1], "events")
        return got

    def feed(self, slices, ev_cap=None, **kw):
        self.deframe_checked(slices, ev_cap)
        return self.account(**kw)

    def close(self):
        self.fc.close()
        self.parser.close()


# ---- replies ---------------------------------------------------------------------------------------------------------
def expected_reply(last, max_frame, routes=None):
    """the oracle's framing of what the model kept -> (wire, slice lengths, counters)"""
    kept, dropped, unrouted = [], 0, 0
    for d, body in last:
        if d[4] != OK:
            dropped += 1
        elif routes is not None and d[3] not in routes:
            unrouted += 1
        else:
            kept.append((body, routes[d[3]] if routes is not None else d[3], d[5] & 1))
    if kept:
        wire, lens = pyorc.h2_frame_batch([k[0] for k in kept], [k[1] for k in kept], [k[2] for k in kept], max_frame)
    else:
        wire, lens = b"", []
    return wire, lens, {"kept": len(kept), "dropped_status": dropped, "unrouted": unrouted}


class Target:
    """slice table and header arena for one framing, sentinel-filled, with room behind the caps"""

    def __init__(self, g, cap):
        self.g, self.cap = g, cap
        self.slices = g.DeviceBuffer(data=bytes([SENTINEL]) * (16 * (cap + 4)))
        self.hdr = g.DeviceBuffer(data=bytes([SENTINEL]) * (32 * (cap + 4)))

    def frame(self, reply, cap=None, hdr_cap=None):
        cap = self.cap if cap is None else cap
        return reply.frame(self.slices.ptr, cap, self.hdr.ptr, 32 * cap if hdr_cap is None else hdr_cap)

    def wire(self, n):
        got = read_slices(self.g, self.slices, n)
        return [ln for _, ln in got], b"".join(device_bytes(self.g, p, ln) for p, ln in got), got


def check_framed(n, st, got_lens, got_wire, expected, what="reply"):
    """one framed reply -- slice count n, stats st, the slice lengths and wire read back -- against expected_reply()'s"""
    wire, lens, counters = expected
    same((n, st["slices"], got_lens), (len(lens), len(lens), lens), what + ": slices (count, stats, lengths)")
    same(got_wire, wire, what + ": wire")
    same(st["wire_bytes"], len(wire), what + ": wire_bytes")
    same({k: st[k] for k in counters}, counters, what + ": counters")
    same((st["overflow"], st["hdr_bytes"] <= 32 * n), (0, True), what + ": (overflow, hdr_bytes %d <= 32 n)" % st["hdr_bytes"])


def check_reply(g, h, reply, max_frame, routes=None):
    """frame the last call of h and compare with the oracle; -> (slices [(ptr, len)], wire)"""
    expected = expected_reply(h.last, max_frame, routes)
    t = h.target = Target(g, len(expected[1]) + 1)  # (the header slices live in it: kept while the harness lives)
    n, st = t.frame(reply)
    got_lens, got_wire, got = t.wire(n)
    print("reply: %d descriptors -> kept %d, %d slices, %d wire bytes, %d us" %
          (len(h.last), st["kept"], n, st["wire_bytes"], st["frame_us"]))
    check_framed(n, st, got_lens, got_wire, expected)
    return got, got_wire


# ---- wire generators (seeded: tests/test_h2_device_lib.py pins their outputs) ----------------------------------------
def sender_slices(sizes, sid=1, end_stream=True, seed=0):
    """Slices as chttp2 hands them to the endpoint: the message header rides in the inlined slice of the
    first frame header (grpc_slice_buffer_add merge), payload slices by reference."""
    out = []
    for i, n in enumerate(sizes):
        body = grpc_msg(bytes((j * 13 + i + seed) % 251 for j in range(n)))
        off = 0
        while off < len(body):
            k = min(16384, len(body) - off)
            last = end_stream and i == len(sizes) - 1 and off + k == len(body)
            fh = k.to_bytes(3, "big") + bytes([0, 1 if last else 0]) + sid.to_bytes(4, "big")
            if off == 0:
                out.append(fh + body[:5])
                if k > 5:
                    out.append(body[5:k])
            else:
                out += [fh, body[off:off + k]]
            off += k
    return out


def fast_sender_slices(sizes, sid=1, seed=0, max_frame=16384):
    """sender_slices with numpy payloads (thousands of slices), any max_frame, no END_STREAM."""
    import numpy as np
    out = []
    for i, n in enumerate(sizes):
        pay = ((np.arange(n, dtype=np.uint32) * 13 + i + seed) % 251).astype(np.uint8).tobytes()
        body = b"\x00" + n.to_bytes(4, "big") + pay
        off = 0
        while off < len(body):
            k = min(max_frame, len(body) - off)
            fh = k.to_bytes(3, "big") + bytes([0, 0]) + sid.to_bytes(4, "big")
            if off == 0:
                out.append(fh + body[:5])
                if k > 5:
                    out.append(body[5:k])
            else:
                out += [fh, body[off:off + k]]
            off += k
    return out


def receiver_slices(tx, first=256):
    """What endpoint reads deliver for those records (rdma_bp_posix.cc:180-326): a read sized to
    max(256, first record) takes whole records and a piece of the next, the following read its rest."""
    out, cur, room = [], b"", first
    for rec in tx:
        while rec:
            if room == 0:
                out.append(cur)
                cur, room = b"", first
            if not cur and len(rec) > first:
                out.append(rec)  # a read sized to the record itself
                rec = b""
                continue
            take = rec[:room]
            cur += take
            room -= len(take)
            rec = rec[len(take):]
            if room == 0 and rec:
                out.append(cur)
                out.append(rec)  # the next read is sized to what is left of the record
                cur, room, rec = b"", first, b""
    if cur:
        out.append(cur)
    return out


def cut_points(data, rng, k):
    """data cut at k random points (fewer where it is shorter)"""
    cuts = sorted(rng.sample(range(1, len(data)), min(k, len(data) - 1)))
    bounds = [0] + cuts + [len(data)]
    return [data[a:b] for a, b in zip(bounds, bounds[1:])]


def cut_mean(data, rng, mean=40):
    """data cut into pieces of exponentially distributed lengths"""
    out, pos = [], 0
    while pos < len(data):
        n = max(1, int(rng.expovariate(1.0 / mean)))
        out.append(data[pos:pos + n])
        pos += n
    return out


def _batch(lens, max_frame, seed):
    rng = random.Random(seed)
    bodies = [(bytes(rng.getrandbits(8) for _ in range(min(n, 4096))) * (n // 4096 + 1))[:n] for n in lens]
    sids = [1] * len(lens)
    flags = [rng.randrange(2) for _ in lens]
    wire, slens = pyorc.h2_frame_batch(bodies, sids, flags, max_frame)
    slices, o = [], 0
    for n in slens:
        slices.append(wire[o:o + n])
        o += n
    return bodies, wire, slices


BATCHES = [([1 << 20], 16384), ([0], 16384), ([0, 0, 0, 5, 0, 0], 16384), ([3, 70000, 16379, 16380], 16384),
           ([100, 0, 17], 3), ([9, 1, 0, 0], 1), ([5000] * 40, 1000), ([1048580] * 3, 16384),
           ([0] * 300 + [7] * 10, 16384), ([20, 0, 21, 22, 0, 0, 23, 24], 5), ([7] * 4200 + [0, 9, 0, 0, 40000], 16384)]


def _eight_streams(seed, nmsg=4, calls=5):
    rng = random.Random(seed)
    sids = list(range(1, 17, 2))
    wire = bytearray(PREFACE + frame(4, 0, 0))
    for s in sids:
        wire += frame(1, 4, s, b"\x82\x86")
    queues = {s: b"".join(grpc_msg(bytes(rng.getrandbits(8) for _ in range(rng.choice([0, 10, 3000, 40000]))))
                          for _ in range(nmsg)) for s in sids}
    while any(queues.values()):
        s = rng.choice([s for s in sids if queues[s]])
        n = rng.randrange(1, 16385)
        part, queues[s] = queues[s][:n], queues[s][n:]
        wire += frame(0, 1 if not queues[s] else 0, s, part)
    wire = bytes(wire)
    cuts = sorted(rng.sample(range(1, len(wire)), calls - 1))
    bounds = [0] + cuts + [len(wire)]
    return wire, [wire[a:b] for a, b in zip(bounds, bounds[1:])]


def _client_stream(seed, sids, nmsg):
    """DATA frames of several opened streams interleaved, some messages cut over frames, one stream ended"""
    rng = random.Random(seed)
    wire = bytearray()
    for k in range(nmsg):
        sid = sids[k % len(sids)]
        body = grpc_msg(bytes(rng.getrandbits(8) for _ in range(rng.choice([0, 1, 5, 300, 5000, 20000]))), k & 1)
        last = k >= nmsg - len(sids) and sid == sids[0]
        for off in range(0, len(body), 16384):
            part = body[off:off + 16384]
            wire += frame(0, 1 if last and off + 16384 >= len(body) else 0, sid, part)
        if k % 3 == 1:
            wire += frame(6, 0, 0, b"12345678") + frame(8, 0, sid, b"\0\0\4\0")
    return bytes(wire)


def _eight_transports(g, seed):
    rng = random.Random(seed)
    ts = []
    for i, vec in enumerate(VEC[:3]):  # the reference's own byte vectors, on fresh server connections
        ts.append(Transport(g, "vec:" + vec["name"], True, cut_points(bytes.fromhex(vec["hex"]), rng, [3, 11, 40][i])))
    ts.append(Transport(g, "client-a", False, cut_points(_client_stream(seed + 1, [1, 3, 5], 9), rng, 14), streams=[1, 3, 5]))
    ts.append(Transport(g, "client-b", False, cut_points(_client_stream(seed + 2, [7], 6), rng, 2), streams=[7]))
    for k in (0, 1):  # eight interleaved streams each, opened by HEADERS frames behind the preface
        wire, _parts = _eight_streams(seed + 10 + k, nmsg=2)
        ts.append(Transport(g, "eight-%d" % k, True, cut_points(wire, rng, 25)))
    ts.append(Transport(g, "empty", False, [], streams=[1]))
    return ts


def _interleaved(seed, sids, sizes):
    """DATA frames of mixed sizes, the streams interleaved"""
    out = []
    for i, n in enumerate(sizes):
        sid = sids[(i * 7 + seed) % len(sids)]
        out.append(frame(0, 0, sid, bytes((i + j) % 251 for j in range(n))))
    return out


FLOW_SIZES = [5, 1000, 16384, 0, 300, 9000, 1, 16384, 77, 4000, 0, 12000]


def _server_open(sids):
    return [PREFACE + frame(4, 0, 0)] + [frame(1, 4, s, b"\x82\x86") for s in sids]


def _dropped_slices():
    """OK, TOO_LARGE, TRUNCATED and NO_SPACE in one call (at max_msg 1200 and a 4096-byte ring): empty kept messages behind
    dropped ones"""
    part = grpc_msg(b"t" * 800)[:500]
    return [frame(0, 0, 1, grpc_msg(b"")), frame(0, 0, 1, grpc_msg(b"L" * 2000)), frame(0, 0, 1, grpc_msg(b"a" * 1000, 1)),
            frame(0, 0, 3, part), frame(3, 0, 3, (8).to_bytes(4, "big")), frame(0, 0, 1, grpc_msg(b"")),
            frame(0, 0, 1, grpc_msg(b"")), frame(0, 0, 1, grpc_msg(b"b" * 1100)), frame(0, 0, 1, grpc_msg(b"c" * 1000)),
            frame(0, 0, 1, grpc_msg(b"d" * 10))]


def _server_call():
    """a server connection opens three streams; END_STREAM, RST_STREAM mid-call and DATA on ids the map does not hold"""
    big = grpc_msg(b"q" * 9000)
    return _server_open((1, 3, 5)) + [
        frame(0, 0, 1, grpc_msg(b"a" * 100)), frame(0, 0, 3, grpc_msg(b"b" * 3000)),
        frame(0, 1, 1, grpc_msg(b"c" * 50)),                       # END_STREAM: no frame for 1, its bytes in the connection's
        frame(0, 0, 5, big[:4000]), frame(3, 0, 5, (8).to_bytes(4, "big")),   # RST_STREAM mid-call
        frame(0, 0, 5, b"x" * 10),                                 # ... and DATA behind it: connection only
        frame(0, 0, 99, b"y" * 700),                               # an unknown stream: connection only
        frame(0, 0, 3, b"")]


# ---- single-link jobs ------------------------------------------------------------------------------------------------
def _pipe_setup(g, h2dev, gs, sizes, npipes, parser):
    from grpc_rdma_amd import h2 as h2host
    bufs = [g.DeviceBuffer(data=bytes((j * 7 + i) % 251 for j in range(n))) for i, n in enumerate(sizes)]
    msgs = [(b.ptr, n, 1, 0) for b, n in zip(bufs, sizes)]
    lens = []
    for n in sizes:
        lens += [len(it[1]) if it[0] == "inl" else it[1][1] for it in h2host.frame_message(n, 1, 16384)]
    scratch = g.DeviceBuffer(nbytes=max(lens) + 64)
    sge = [(scratch.ptr, n) for n in lens]
    tx, rx = g.Pair(1 << 18, 30), g.Pair(1 << 18, 30)
    g.connect_pairs(tx, rx)
    N = sum(lens)
    scap = 2 * len(lens) + 64 + N // 256
    dst_cap = N + 16 * scap + 4096
    keep = [bufs, scratch, tx, rx]
    pipes, jobs = [], []
    for _ in range(npipes):
        dst = g.DeviceBuffer(nbytes=dst_cap)
        job = gs.StreamJob(tx, rx, sge, dst.ptr, dst_cap, scap, 64)
        r = job.run(gs.RUN_EAGER)
        job.set_rounds(int(max(r.tx_rounds, r.rx_rounds)))
        r = job.run(gs.RUN_GRAPH)
        same((bool(r.done), int(r.bytes_delivered)), (True, N), "recorded run (done, bytes delivered)")
        pipes.append(h2dev.Pipe(job, msgs, parser, len(job.delivered_slices(0)), 4 * len(lens) + 256))
        jobs.append(job)
        keep.append(dst)
    return pipes, jobs, keep


def _back_job(g, gs, lens):
    """a job over a connection of its own whose recorded run carries slices of the lengths `lens`"""
    scratch = g.DeviceBuffer(nbytes=max(lens) + 64)
    sge = [(scratch.ptr, n) for n in lens]
    tx, rx = g.Pair(1 << 18, 30), g.Pair(1 << 18, 30)
    g.connect_pairs(tx, rx)
    N = sum(lens)
    scap = 2 * len(lens) + 64 + N // 256
    dst_cap = N + 16 * scap + 4096
    dst = g.DeviceBuffer(nbytes=dst_cap)
    job = gs.StreamJob(tx, rx, sge, dst.ptr, dst_cap, scap, 64)
    r = job.run(gs.RUN_EAGER)
    job.set_rounds(int(max(r.tx_rounds, r.rx_rounds)))
    r = job.run(gs.RUN_GRAPH)
    same((bool(r.done), int(r.bytes_delivered), int(r.bytes_sent)), (True, N, N), "recorded run (done, delivered, sent)")
    return job, lens, int(r.bytes_sent), [scratch, tx, rx, dst]


# ---- the four-link job of the group pipes ----------------------------------------------------------------------------
LINK_SIZES = [0, 1, 5, 16379, 16380, 70000, 200000]
# per link: (length, stream id, flags); counts differ (five is no multiple of four), a run of empty messages in front of
# a non-empty one, one stream ended by its last message (links 2 and 3 are the two directions of one pair)
TABLES = [
    [(16380, 1, 0), (0, 1, 1), (0, 3, 0), (0, 1, 0), (5, 3, 1), (200000, 1, 0), (1, 3, 0), (16379, 1, 1)],
    [(70000, 5, 1), (1, 5, 0), (16379, 5, 0), (0, 5, 0), (5, 5, 0)],
    [(5, 7, 0), (200000, 9, 1), (16380, 7, 0), (0, 9, 0), (0, 9, 0), (70000, 7, 0)],
    [(0, 2, 0), (16379, 2, 0), (1, 4, 1), (70000, 4, 0), (0, 2, 0), (5, 4, 0), (16380, 2, 2)],
]
assert all(n in LINK_SIZES for t in TABLES for n, _, _ in t) and {n for t in TABLES for n, _, _ in t} == set(LINK_SIZES)


def _body(li, k, n):
    return bytes((j * (7 + 2 * li) + 13 * k + li) % 251 for j in range(n))


class Links:
    """a MultiStreamJob of four links over 256 KiB rings, run once over slice lists of the framed tables' lengths
    (TABLES is read when an instance is built: a test that wants other stream ids patches this module's TABLES)"""

    def __init__(self, g, max_frame=16384, pipeline=False):
        from grpc_rdma_amd import stream as gs
        self.g, self.max_frame = g, max_frame
        R, max_sge = 1 << 18, 30
        p0a, p0b, p1a, p1b, p2a, p2b = [g.Pair(R, max_sge) for _ in range(6)]
        g.connect_pairs(p0a, p0b)
        g.connect_pairs(p1a, p1b)
        g.connect_pairs(p2a, p2b)
        self.pairs = [p0a, p0b, p1a, p1b, p2a, p2b]
        ends = [(p0a, p0b), (p1a, p1b), (p2a, p2b), (p2b, p2a)]
        self.bodies, self.msgs, self.wire, self.lens, self.dsts, self.keep, specs = [], [], [], [], [], [], []
        for li, tab in enumerate(TABLES):
            bodies = [_body(li, k, n) for k, (n, _, _) in enumerate(tab)]
            bufs = [g.DeviceBuffer(data=b, offset=(3 * k + li) % 16) if b else g.DeviceBuffer(nbytes=1) for k, b in enumerate(bodies)]
            wire, lens = pyorc.h2_frame_batch(bodies, [s for _, s, _ in tab], [f for _, _, f in tab], max_frame)
            # the recorded run carries placeholders of the right lengths (a pattern of the link's own)
            scratch = g.DeviceBuffer(data=bytes((j * 5 + li) % 253 for j in range(max(lens) + 64)))
            N = sum(lens)
            scap = 2 * len(lens) + 64 + N // 256
            dcap = N + 16 * scap + 4096
            dst = g.DeviceBuffer(nbytes=dcap)
            specs.append((ends[li][0], ends[li][1], [(scratch.ptr, n) for n in lens], dst.ptr, dcap, scap))
            self.keep.append((bufs, scratch))
            self.bodies.append(bodies)
            self.msgs.append([(b.ptr, n, s, f) for b, (n, s, f) in zip(bufs, tab)])
            self.wire.append(wire)
            self.lens.append(lens)
            self.dsts.append((dst, dcap))
        self.job = gs.MultiStreamJob(specs, 256)
        self.job.set_pipeline(pipeline)   # (paired schedule: the graph is built by another branch of the job)
        r = self.job.run(gs.RUN_EAGER)
        same(bool(r.done), True, "recorded eager run done")
        n_rounds = int(max(r.tx_rounds, r.rx_rounds))
        self.job.set_rounds(2 * n_rounds + 4 if pipeline else n_rounds + 2)
        r = self.job.run(gs.RUN_GRAPH)
        same((bool(r.done), int(r.bytes_delivered)), (True, sum(sum(x) for x in self.lens)), "recorded graph run (done, bytes)")
        self.recorded = [self.delivered(li) for li in range(4)]

    def delivered(self, li):
        dst, dcap = self.dsts[li]
        mem = dst.read(dcap)
        return [mem[o:o + n] for o, n in self.job.delivered_slices(li)]

    def streams(self, li):
        return sorted({s for _, s, _ in TABLES[li]})

    def parser(self, li):
        """(device parser, oracle parser) of link li, its table's streams opened on both"""
        pp = ParserPair(self.g, False, self.streams(li), self.max_frame)
        return pp.dev, pp.orc

    def spec(self, li, parser):
        return (li, self.msgs[li], parser, len(self.recorded[li]), 4 * len(self.lens[li]) + 256)

    def close(self):
        self.job.close()
        for p in self.pairs:
            p.close()


@pytest.fixture(params=["fused", "stages"])
def fused(request, monkeypatch):
    monkeypatch.setenv("GRDMA_H2_PIPE_FUSED", "1" if request.param == "fused" else "0")
    return request.param == "fused"


def step_events(orc, delivered, what):
    """an oracle parser takes the slices one step delivered -> the events; the step has no h2 error"""
    err, ev = oracle_feed(orc, delivered)
    same(err, 0, "%r: the oracle's h2 error" % (what,))
    return ev


def _check_steps(L, gp, listed, parsers, steps):
    for step in range(steps):
        gp.enqueue()
        res = gp.sync()
        for i, li in enumerate(listed):
            r, what = res[i], "step %d link %d" % (step, li)
            same((r["frame_overflow"], r["deframe_overflow"], r["h2_error"]), (0, 0, 0),
                 what + " (frame_overflow, deframe_overflow, h2_error) of %r" % (r,))
            table = gp.slice_table(i)
            same((r["framed"], len(table)), (len(L.lens[li]),) * 2, what + " (framed, slice table length)")
            same([n for _, n in table], L.lens[li], what + " slice lengths")
            same(b"".join(device_bytes(L.g, p, n) for p, n in table), L.wire[li], what + " gathered wire")
            got = L.delivered(li)
            same(b"".join(got), L.wire[li], what + " delivered bytes")
            same(r["parsed"], len(got), what + " parsed")
            ev_g = gp.events(i)
            same(r["events"], len(ev_g), what + " event count")
            same(ev_g, step_events(parsers[i][1], got, what), what + " events")


class LinkAsm:
    """per listed link: a device assembler, the model, an oracle parser of its own (the events the model is fed) and the
    streams that have closed so far"""

    def __init__(self, L, li, parser):
        from grpc_rdma_amd import h2dev
        self.li = li
        self.arena = L.g.DeviceBuffer(data=bytes([SENTINEL]) * (1 << 20))
        self.asm = h2dev.Assembler(parser, self.arena)
        self.model = AsmModel(1 << 20)
        self.orc = oracle_parser(False, L.max_frame, L.streams(li))
        self.closed = set()

    def advance(self, delivered, what):
        """the oracle parser and the model take one step over `delivered` -> (events, the model's [(descriptor, bytes)])"""
        ev = step_events(self.orc, delivered, what)
        self.model.release()   # (a step first releases everything reported before it)
        return ev, self.model.call(ev, delivered, 0)

    def check_step(self, L, msgs, what):
        """msgs = the group pipe's descriptors of this link for the step that just ended"""
        ev, exp = self.advance(L.delivered(self.li), what)
        same([tuple(m) for m in msgs], [d for d, _ in exp], "%r descriptors" % (what,))
        same([m.status for m in msgs], [OK] * len(msgs), "%r statuses" % (what,))
        # the bodies that were framed, on the streams still open when the step began
        framed = [(s, b) for (_, s, _), b in zip(TABLES[self.li], L.bodies[self.li]) if s not in self.closed]
        same([(m.stream_id, self.asm.view(m)) for m in msgs], framed, "%r (stream, bytes in the arena)" % (what,))
        same([b for _, b in exp], [b for _, b in framed], "%r the model's bodies" % (what,))
        self.closed |= {e[3] for e in ev if e[0] == pyorc.EV_STREAM_CLOSED}


# ---- the echo over two four-link jobs --------------------------------------------------------------------------------
ROUTES3 = {4: 44}   # link 3: stream 2 ends with its last message of the first step; only stream 4 is sent back


class BackLinks:
    """a MultiStreamJob of len(lens) links, each over a pair of its own, run once over slice lists of the lengths `lens`"""

    def __init__(self, g, lens):
        from grpc_rdma_amd import stream as gs
        self.g, self.lens, self.pairs, self.dsts, self.keep, specs = g, lens, [], [], [], []
        for li, ln in enumerate(lens):
            a, b = g.Pair(1 << 18, 30), g.Pair(1 << 18, 30)
            g.connect_pairs(a, b)
            self.pairs += [a, b]
            scratch = g.DeviceBuffer(data=bytes((j * 3 + li) % 249 for j in range(max(ln) + 64)))
            N = sum(ln)
            scap = 2 * len(ln) + 64 + N // 256
            dcap = N + 16 * scap + 4096
            dst = g.DeviceBuffer(nbytes=dcap)
            specs.append((a, b, [(scratch.ptr, n) for n in ln], dst.ptr, dcap, scap))
            self.dsts.append((dst, dcap))
            self.keep.append(scratch)
        self.job = gs.MultiStreamJob(specs, 256)
        self.job.set_pipeline(False)
        r = self.job.run(gs.RUN_EAGER)
        same(bool(r.done), True, "recorded eager run done")
        self.job.set_rounds(int(max(r.tx_rounds, r.rx_rounds)) + 2)
        r = self.job.run(gs.RUN_GRAPH)
        same((bool(r.done), int(r.bytes_delivered)), (True, sum(sum(x) for x in lens)), "recorded graph run (done, bytes)")
        self.recorded = [len(self.job.delivered_slices(li)) for li in range(len(lens))]

    def close(self):
        self.job.close()
        for p in self.pairs:
            p.close()


class Echo:
    """forward: a Links job with a GroupPipe and an assembler on each of its four links; back: a job of four links with
    a group reply pipe whose spec i frames what forward link i assembled, back parsers and back assemblers attached"""

    def __init__(self, g):
        from grpc_rdma_amd import h2dev
        self.g = g
        L = self.L = Links(g)
        self.parsers = [L.parser(li) for li in range(4)]
        self.gp = h2dev.GroupPipe(L.job, [L.spec(li, self.parsers[li][0]) for li in range(4)])
        self.las = [LinkAsm(L, li, self.parsers[li][0]) for li in range(4)]
        self.gp.attach_assemblers([la.asm for la in self.las])
        self.routes = [None, None, None, ROUTES3]
        self.replies = [h2dev.Reply(la.asm, list(r.items()) if r else None, 16384, 64) for la, r in zip(self.las, self.routes)]
        # what comes back per link: the oracle's framing of the kept messages (compressed flag passed through)
        self.back, self.wire, self.lens = [], [], []
        for li, tab in enumerate(TABLES):
            r = self.routes[li]
            kept = [(b, r[s] if r else s, f & 1) for (_, s, f), b in zip(tab, L.bodies[li]) if r is None or s in r]
            wire, lens = pyorc.h2_frame_batch([k[0] for k in kept], [k[1] for k in kept], [k[2] for k in kept], 16384)
            self.back.append(kept)
            self.wire.append(wire)
            self.lens.append(lens)
        same([len(k) for k in self.back], [len(t) for t in TABLES[:3]] + [3], "messages kept per link")
        self.B = BackLinks(g, self.lens)
        self.parsers_back = []
        for kept in self.back:
            p = h2dev.Parser(False, 16384)
            same(p.open_streams(sorted({s for _, s, _ in kept})), 0, "open_streams of a back parser")
            self.parsers_back.append(p)
        self.rspecs = [(li, self.replies[li], self.parsers_back[li], self.B.recorded[li], 4 * len(self.lens[li]) + 256,
                        sum(self.lens[li])) for li in range(4)]
        self.arenas_back = [g.DeviceBuffer(nbytes=1 << 20) for _ in range(4)]
        self.asms_back = [h2dev.Assembler(p, a) for p, a in zip(self.parsers_back, self.arenas_back)]
        self.seq_back = [0] * 4
        self.rp = None

    def advance(self, li, delivered):
        """link li's oracle parser and model take one step over `delivered` -> the model's descriptors"""
        return [d for d, _ in self.las[li].advance(delivered, ("advance", li))[1]]

    def forward_checked(self, what, overwritten=()):
        """the forward step that was enqueued last has ended: per link the descriptors and bytes equal the model's
        (overwritten: links whose assembler has taken another pipe's step since -- their models follow unchecked)"""
        fr = self.gp.sync()
        for li, la in enumerate(self.las):
            same((fr[li]["h2_error"], fr[li]["frame_overflow"]), (0, 0), "%r forward link %d (h2_error, frame_overflow)" % (what, li))
            if li in overwritten:
                self.advance(li, self.L.delivered(li))
                continue
            la.check_step(self.L, self.gp.messages(li), (what, li))
            step_bytes = sum(((n + 255) // 256) * 256 for n, _, _ in TABLES[li])
            in_use, most = la.asm.stats()["bytes_in_use"], step_bytes + max(n for n, _, _ in TABLES[li])
            same(in_use <= most, True, "%r forward link %d: %d bytes in use, at most %d" % (what, li, in_use, most))

    def back_checked(self, res, li, what):
        """link li of the reply step that was synced as `res` delivered the forward bodies"""
        r, what = res[li], "%r back link %d" % (what, li)
        same((r["h2_error"], r["frame_overflow"], r["framed"]), (0, 0, len(self.lens[li])),
             what + " (h2_error, frame_overflow, framed) of %r" % (r,))
        got = self.rp.messages(li)
        kept = self.back[li]
        same([(m.status, m.length, m.stream_id, m.flags) for m in got], [(OK, len(b), s, f) for b, s, f in kept],
             what + " (status, length, stream, flags)")
        same([m.seq for m in got], list(range(self.seq_back[li], self.seq_back[li] + len(kept))), what + " seqs")
        self.seq_back[li] += len(kept)
        same([self.asms_back[li].view(m) for m in got], [b for b, _, _ in kept], what + " bodies")
        table = self.rp.slice_table(li)
        same([n for _, n in table], self.lens[li], what + " slice lengths")
        same(b"".join(device_bytes(self.g, p, n) for p, n in table), self.wire[li], what + " gathered wire")
        return table

    def step(self, what):
        self.gp.enqueue()
        self.rp.enqueue()
        res = self.rp.sync()
        tables = [self.back_checked(res, li, what) for li in range(4)]
        self.forward_checked(what)
        return tables

    def close(self):
        from grpc_rdma_amd import h2dev
        if self.rp:
            self.rp.close()
        self.gp.close()
        same(self.gp.h, None, "the forward group pipe's handle after close")
        same((h2dev.job_hook_counts(self.B.job), h2dev.job_hook_counts(self.L.job)), ((0, 0), (0, 0)), "job hooks after close")
        for r in self.replies:
            r.close()
        for a in self.asms_back + [la.asm for la in self.las]:
            a.close()
        for p in self.parsers_back + [p for p, _ in self.parsers]:
            p.close()
        self.B.close()
        self.L.close()
