"""What the call table's tests share (tests/test_zz_gpu_h2_calls.py, the sweep, tools/h2_calls_probe.py): the harness of
the device tests -- a device table (h2dev.CallTable) and the model of tests/h2_calls_model.py beside it, every step
compared whole: the dispatch table, the segment words, the done list, the result block, the dump and the counters.
What a step does not write keeps its fill.  pytest rewrites no `assert` in a helper module: every check goes through
`same`."""
import struct

from tests.h2_calls_model import CallsModel, dispatch_bytes, done_bytes, entry_bytes
from tests.h2_hpenc_lib import ERR2, ERR5, SENTINEL

BIG = 1 << 40


def blocks_bytes(blocks):
    return b"".join(struct.pack("<4I", *b) for b in blocks)


def meta_bytes(meta):
    return b"".join(struct.pack("<12I", *r) for r in meta)


def msgs_bytes(msgs):
    return b"".join(struct.pack("<QQQIIII", *m, 0) for m in msgs)


def events_bytes(events):
    return b"".join(struct.pack("<6I", *e) for e in events)


class Tables:
    """a step's four input tables in device memory"""

    def __init__(self, g, blocks, meta, msgs, events):
        self.n = (len(blocks), len(msgs), len(events))
        self.blocks = g.DeviceBuffer(data=blocks_bytes(blocks) + bytes(16))
        self.meta = g.DeviceBuffer(data=meta_bytes(meta) + bytes(48))
        self.msgs = g.DeviceBuffer(data=msgs_bytes(msgs) + bytes(40))
        self.events = g.DeviceBuffer(data=events_bytes(events) + bytes(24))

    def args(self):
        return (self.blocks.ptr, self.meta.ptr, self.n[0], self.msgs.ptr, self.n[1], self.events.ptr, self.n[2])


class Out:
    """a dispatch table, the segment words and a done list filled with SENTINEL, with room behind the caps"""

    def __init__(self, g, dispatch_cap, done_cap, nmethods):
        self.caps = (dispatch_cap, done_cap)
        self.dispatch = g.DeviceBuffer(data=bytes([SENTINEL]) * (48 * (dispatch_cap + 2)))
        self.segments = g.DeviceBuffer(data=bytes([SENTINEL]) * (4 * (nmethods + 2 + 4)))
        self.done = g.DeviceBuffer(data=bytes([SENTINEL]) * (32 * (done_cap + 2)))

    def args(self):
        return (self.dispatch.ptr, self.caps[0], self.segments.ptr, self.done.ptr, self.caps[1])


def filled(want, n):
    return want + bytes([SENTINEL]) * (n - len(want))


class CH:
    def __init__(self, g, table_slots=0, nmethods=1):
        from grpc_rdma_amd import h2dev
        self.g = g
        self.nmethods = nmethods
        self.dev = h2dev.CallTable(table_slots, nmethods)
        self.model = CallsModel(table_slots, nmethods)
        self.check()

    def step(self, reqs=(), msgs=(), events=(), now=0, dispatch_cap=None, done_cap=None, device=None):
        """one step on the device and in the model, everything compared -> (dispatch records, segment words, done
        records, result tuple).  reqs: [(block, call record)] (h2_calls_model.request); the caps default to what the
        step needs and one more.  device: the seven input arguments where the tables stand in device memory already
        (reqs, msgs, events: what they hold)"""
        import copy
        import pytest
        from tests.h2_device_lib import same
        blocks, meta = [r[0] for r in reqs], [r[1] for r in reqs]
        msgs, events = list(msgs), list(events)
        if dispatch_cap is None or done_cap is None:
            need = copy.deepcopy(self.model).step(blocks, meta, msgs, events, now, BIG, BIG)[3]
            dispatch_cap = len(msgs) + 1 if dispatch_cap is None else dispatch_cap
            done_cap = need[3] + 1 if done_cap is None else done_cap
        disp, segs, done, res, err = self.model.step(blocks, meta, msgs, events, now, dispatch_cap, done_cap)
        inp = None if device else Tables(self.g, blocks, meta, msgs, events)
        out = Out(self.g, max(1, dispatch_cap), max(1, done_cap), self.nmethods)
        args = tuple(device or inp.args()) + (now,) + out.args()
        if err:
            with pytest.raises(self.g.GrdmaError, match=ERR5 if err == "capacity" else ERR2):
                self.dev.step(*args)
            got = self.dev.last_result
        else:
            n, got = self.dev.step(*args)
            same(n, len(msgs), "step: the number of dispatch records")
        print("step: %r -> %r" % (res, got))
        same(got, res, "step: result")
        d, s, f = out.dispatch.read(), out.segments.read(), out.done.read()
        for k, x in enumerate(disp):  # (say which record, then fail on the bytes)
            if d[48 * k:48 * k + 48] != dispatch_bytes(x):
                same(struct.unpack("<QQQIIIIII", d[48 * k:48 * k + 48]), x, "step: dispatch record %d" % k)
        same(d, filled(b"".join(dispatch_bytes(x) for x in disp), len(d)), "step: the whole dispatch table")
        same(s, filled(b"" if segs is None else struct.pack("<%dI" % len(segs), *segs), len(s)), "step: the segment words")
        for k, x in enumerate(done):
            if f[32 * k:32 * k + 32] != done_bytes(x):
                same(struct.unpack("<QQIIII", f[32 * k:32 * k + 32]), x, "step: done record %d" % k)
        same(f, filled(b"".join(done_bytes(x) for x in done), len(f)), "step: the whole done list")
        self.check()
        return disp, segs, done, res

    def check(self):
        from tests.h2_device_lib import same
        st = self.dev.stats()
        same({k: st[k] for k in self.model.stats}, self.model.stats, "counters (all: %r)" % (st,))
        entries, (n, serial, slots) = self.dev.dump()
        want = self.model.dump()
        same(entries.tobytes(), b"".join(entry_bytes(r) for r in want), "the dump")
        same((n, serial, slots), (len(want), self.model.serial, self.model.slots), "the dump's words")

    def close(self):
        self.dev.close()


def cluster_id(home, k, slots=16):
    """the k-th stream id whose home slot in a table of `slots` is `home` (the stream-table tests' construction)"""
    return 2 * (home + slots * k) + 1
