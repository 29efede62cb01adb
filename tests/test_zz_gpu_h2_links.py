"""HTTP/2 on every link of a multi-connection job: the batched deframer (grdma_h2_deframe_batch, k_h2_deframe_links) and
the group pipe (grdma_h2_group_pipe: k_h2_frame_links -> MultiStreamJob -> k_h2_deframe_links).  The reference is the
oracle everywhere -- pyorc.H2Parser fed the bytes of the delivered slices, pyorc.h2_frame_batch for wire and slice
lengths -- and every comparison is exact.  The cases are small enough for the wave emulator (tests/test_h2_links_emu.py)."""
import os
import random

import pytest

from oracle import pyorc
from tests.h2_helpers import PREFACE, frame, grpc_msg
from tests.test_gpu_h2 import VEC, device_bytes, oracle_events, read_slices  # noqa: F401
from tests.test_zz_gpu_h2_messages import _eight_streams

pytestmark = pytest.mark.gpu

ERR_CAPACITY = -5  # -GRDMA_ERR_CAPACITY


def _cut(data, rng, k):
    cuts = sorted(rng.sample(range(1, len(data)), min(k, len(data) - 1)))
    bounds = [0] + cuts + [len(data)]
    return [data[a:b] for a, b in zip(bounds, bounds[1:])]


class Transport:
    """one connection: a device parser, the oracle's parser beside it, and the slices still to be delivered"""

    def __init__(self, g, name, prefix, slices, streams=(), max_frame=16384):
        from grpc_rdma_amd import h2dev
        self.g, self.name, self.prefix, self.streams, self.max_frame = g, name, prefix, tuple(streams), max_frame
        self.slices = list(slices)
        self.dev = h2dev.Parser(prefix, max_frame)
        self.orc = pyorc.H2Parser(expect_client_prefix=prefix, max_frame_size=max_frame)
        if streams:
            assert self.dev.open_streams(streams) == 0
            for s in streams:
                assert self.orc.open_stream(s) == 0
        self.bufs = []

    def item(self, slices, rng=None):
        """(parser, arena ptr, slice table) of one call over `slices`, which go into an arena of their own"""
        arena, table = bytearray(), []
        for s in slices:
            if rng is not None:
                arena += b"\xee" * rng.randrange(1, 16)
            table.append((len(arena), len(s)))
            arena += s + bytes((-len(s)) % 16)
        buf = self.g.DeviceBuffer(data=bytes(arena) + bytes(64))
        self.bufs.append(buf)
        return (self.dev, buf.ptr, table)

    def expect(self, slices):
        """the oracle over the same call: (h2 error, events with the slice index of the call)"""
        out = []
        for i, s in enumerate(slices):
            rc, ev = self.orc.feed(s)
            out += [(k, a, b, c, d, i) for k, a, b, c, d in ev]
            if rc:
                return rc, out
        return 0, out

    def close(self):
        self.dev.close()


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
        ts.append(Transport(g, "vec:" + vec["name"], True, _cut(bytes.fromhex(vec["hex"]), rng, [3, 11, 40][i])))
    ts.append(Transport(g, "client-a", False, _cut(_client_stream(seed + 1, [1, 3, 5], 9), rng, 14), streams=[1, 3, 5]))
    ts.append(Transport(g, "client-b", False, _cut(_client_stream(seed + 2, [7], 6), rng, 2), streams=[7]))
    for k in (0, 1):  # eight interleaved streams each, opened by HEADERS frames behind the preface
        wire, _parts = _eight_streams(seed + 10 + k, nmsg=2)
        ts.append(Transport(g, "eight-%d" % k, True, _cut(wire, rng, 25)))
    ts.append(Transport(g, "empty", False, [], streams=[1]))
    assert len(ts) == 8
    return ts


def _run_batch(ts, halves, order, rng=None):
    """one grdma_h2_deframe_batch over ts in `order`; halves[i] = the slices of transport i in this call"""
    from grpc_rdma_amd import h2dev
    items = [ts[i].item(halves[i], rng) for i in order]
    got = h2dev.deframe_batch(items)
    res = [None] * len(ts)
    for k, i in enumerate(order):
        res[i] = got[k]
    return res


def test_batch_equals_the_oracle_per_transport(gpu):
    """Eight transports in one launch, each with its own bytes, parser and stream map; a second batch with the
    continuation of every stream (state is carried per parser); the same items in another order give the same
    per-item results."""
    results = {}
    for order_seed in (None, 5):
        ts = _eight_transports(gpu, 31)
        order = list(range(8))
        if order_seed is not None:
            random.Random(order_seed).shuffle(order)
            assert order != list(range(8))
        first = [t.slices[:(len(t.slices) + 1) // 2] for t in ts]
        second = [t.slices[(len(t.slices) + 1) // 2:] for t in ts]
        got = []
        for call, halves in enumerate((first, second)):
            res = _run_batch(ts, halves, order, rng=random.Random(call) if order_seed is None else None)
            for i, t in enumerate(ts):
                exp = t.expect(halves[i])
                assert res[i][0] == exp[0] == 0, (t.name, call)
                assert res[i][1] == exp[1], (t.name, call)
            got.append(res)
        assert got[0][7] == (0, []) and got[1][7] == (0, [])  # the empty list
        assert sum(len(r[1]) for r in got[0]) > 200
        for t in ts:
            assert t.dev.live_streams() == t.orc.live_streams(), t.name
            t.close()
        results[order_seed] = got
    assert results[None] == results[5]


def test_errors_and_overflow_stay_with_their_transport(gpu):
    body = bytes(range(200))
    rng = random.Random(9)
    # a frame header longer than the parser's max_frame_size, behind two good frames
    too_large = frame(0, 0, 1, grpc_msg(body)) + frame(0, 0, 1, grpc_msg(b"")) + (16385).to_bytes(3, "big") + bytes([0, 0]) + \
        (1).to_bytes(4, "big") + bytes(50)
    assert oracle_events([too_large], False, streams=(1,))[0] == 2   # GRDMA_H2_ERR_FRAME_TOO_LARGE
    bad_preface = PREFACE[:-1] + b"X" + frame(4, 0, 0)
    assert oracle_events([bad_preface], True)[0] == 1                # GRDMA_H2_ERR_PREFIX
    wire8, _ = _eight_streams(77, nmsg=2)
    ts = [Transport(gpu, "good-a", False, _cut(_client_stream(3, [1, 3], 7), rng, 9), streams=[1, 3]),
          Transport(gpu, "too-large", False, _cut(too_large, rng, 4), streams=[1]),
          Transport(gpu, "good-b", True, _cut(wire8, rng, 12)),
          Transport(gpu, "bad-preface", True, _cut(bad_preface, rng, 2)),
          Transport(gpu, "small-cap", False, _cut(_client_stream(4, [5], 5), rng, 3), streams=[5]),
          Transport(gpu, "good-c", True, _cut(bytes.fromhex(VEC[0]["hex"]), rng, 6))]
    from grpc_rdma_amd import h2dev
    # the good ones keep a tail for a further call
    now = [t.slices[:-2] if t.name.startswith("good") else t.slices for t in ts]
    later = [t.slices[-2:] if t.name.startswith("good") else [] for t in ts]
    items = [t.item(s) for t, s in zip(ts, now)]
    exp = [t.expect(s) for t, s in zip(ts, now)]
    assert len(exp[4][1]) > 4
    caps = [None, None, None, None, 3, None]
    got = h2dev.deframe_batch(items, caps=caps)
    for i, t in enumerate(ts):
        if t.name == "small-cap":
            assert got[i][1] == ERR_CAPACITY
            continue
        assert got[i][0] == exp[i][0], t.name
        assert got[i][1] == exp[i][1], t.name
    assert got[1][0] == 2 and got[3][0] == 1
    for i, t in enumerate(ts):
        if not t.name.startswith("good"):
            continue
        assert t.dev.live_streams() == t.orc.live_streams(), t.name
        parser, arena, table = t.item(later[i])
        err, ev = parser.deframe(arena, table)   # (the single-call kernel on the state the batch left)
        assert (err, ev) == t.expect(later[i]), t.name
        assert t.dev.live_streams() == t.orc.live_streams(), t.name
    for t in ts:
        t.close()


# ---- the group pipe ------------------------------------------------------------------------------------------------
SIZES = [0, 1, 5, 16379, 16380, 70000, 200000]
# per link: (length, stream id, flags); counts differ (five is no multiple of four), a run of empty messages in front of
# a non-empty one, one stream ended by its last message (links 2 and 3 are the two directions of one pair)
TABLES = [
    [(16380, 1, 0), (0, 1, 1), (0, 3, 0), (0, 1, 0), (5, 3, 1), (200000, 1, 0), (1, 3, 0), (16379, 1, 1)],
    [(70000, 5, 1), (1, 5, 0), (16379, 5, 0), (0, 5, 0), (5, 5, 0)],
    [(5, 7, 0), (200000, 9, 1), (16380, 7, 0), (0, 9, 0), (0, 9, 0), (70000, 7, 0)],
    [(0, 2, 0), (16379, 2, 0), (1, 4, 1), (70000, 4, 0), (0, 2, 0), (5, 4, 0), (16380, 2, 2)],
]
assert all(n in SIZES for t in TABLES for n, _, _ in t) and {n for t in TABLES for n, _, _ in t} == set(SIZES)


def _body(li, k, n):
    return bytes((j * (7 + 2 * li) + 13 * k + li) % 251 for j in range(n))


class Links:
    """a MultiStreamJob of four links over 256 KiB rings, run once over slice lists of the framed tables' lengths"""

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
        assert r.done
        n_rounds = int(max(r.tx_rounds, r.rx_rounds))
        self.job.set_rounds(2 * n_rounds + 4 if pipeline else n_rounds + 2)
        r = self.job.run(gs.RUN_GRAPH)
        assert r.done and r.bytes_delivered == sum(sum(x) for x in self.lens)
        self.recorded = [self.delivered(li) for li in range(4)]

    def delivered(self, li):
        dst, dcap = self.dsts[li]
        mem = dst.read(dcap)
        return [mem[o:o + n] for o, n in self.job.delivered_slices(li)]

    def parser(self, li):
        from grpc_rdma_amd import h2dev
        p = h2dev.Parser(False, self.max_frame)
        sids = sorted({s for _, s, _ in TABLES[li]})
        assert p.open_streams(sids) == 0
        o = pyorc.H2Parser(expect_client_prefix=False, max_frame_size=self.max_frame)
        for s in sids:
            assert o.open_stream(s) == 0
        return p, o

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


def _check_steps(L, gp, listed, parsers, steps):
    for step in range(steps):
        gp.enqueue()
        res = gp.sync()
        for i, li in enumerate(listed):
            r = res[i]
            assert r["frame_overflow"] == 0 and r["deframe_overflow"] == 0 and r["h2_error"] == 0, (step, li, r)
            table = gp.slice_table(i)
            assert r["framed"] == len(table) == len(L.lens[li])
            assert [n for _, n in table] == L.lens[li], (step, li)
            assert b"".join(device_bytes(L.g, p, n) for p, n in table) == L.wire[li], (step, li)
            got = L.delivered(li)
            assert b"".join(got) == L.wire[li], (step, li)
            assert r["parsed"] == len(got)
            ev_o = []
            for k, s in enumerate(got):
                rc, ev = parsers[i][1].feed(s)
                assert rc == 0
                ev_o += [(kk, a, b, c, d, k) for kk, a, b, c, d in ev]
            ev_g = gp.events(i)
            assert r["events"] == len(ev_g) and ev_g == ev_o, (step, li)


def test_group_pipe_four_links_five_steps(gpu, fused):
    """Links 2 and 3 are the two directions of one pair.  After every step and per link: the slice table and the bytes
    it gathers equal the oracle's framing, the delivered bytes equal that wire, the events equal one oracle parser per
    link kept across the steps."""
    from grpc_rdma_amd import h2dev
    L = Links(gpu)
    parsers = [L.parser(li) for li in range(4)]
    gp = h2dev.GroupPipe(L.job, [L.spec(li, parsers[li][0]) for li in range(4)])
    assert gp.hook_counts() == ((1, 1) if fused else (0, 0))   # ONE kernel in front, ONE behind, for four links
    _check_steps(L, gp, [0, 1, 2, 3], parsers, 5)
    for li in range(4):
        assert parsers[li][0].live_streams() == parsers[li][1].live_streams()
    gp.close()
    assert h2dev.job_hook_counts(L.job) == (0, 0)
    for p, _ in parsers:
        p.close()
    L.close()


def test_group_pipe_on_a_pipelined_job_parses_what_the_step_delivered(gpu, fused):
    """The shape the group pipe is for: a pipelined (paired schedule) job with a bidirectional pair.  The deframing
    kernel reads the slice count the job's drain leaves on the device for THIS step -- at small rings a step may deliver
    a slice more or less than the recorded run -- so the count handed to create is no input of the parse: with counts
    that are off by one, two and many the events still equal the oracle's over everything the step delivered."""
    from grpc_rdma_amd import h2dev
    L = Links(gpu, pipeline=True)
    parsers = [L.parser(li) for li in range(4)]
    specs = [L.spec(li, parsers[li][0]) for li in range(4)]
    off = [-1, 2, 0, -len(L.recorded[3]) + 1]
    specs = [(li, m, p, n + d, cap) for (li, m, p, n, cap), d in zip(specs, off)]
    gp = h2dev.GroupPipe(L.job, specs)
    _check_steps(L, gp, [0, 1, 2, 3], parsers, 3)
    gp.close()
    for p, _ in parsers:
        p.close()
    L.close()


def test_one_launch_per_step_in_fused_mode(gpu, monkeypatch):
    """The job's graph carries ONE kernel in front of and ONE behind its rounds for four links -- a step is one graph
    launch -- and none once the pipe is closed; with GRDMA_H2_PIPE_FUSED=0 it carries none at all."""
    from grpc_rdma_amd import h2dev
    L = Links(gpu)
    parsers = [L.parser(li) for li in range(4)]
    for env, want in (("1", (1, 1)), ("0", (0, 0)), (None, (1, 1))):
        if env is None:
            monkeypatch.delenv("GRDMA_H2_PIPE_FUSED", raising=False)
        else:
            monkeypatch.setenv("GRDMA_H2_PIPE_FUSED", env)
        gp = h2dev.GroupPipe(L.job, [L.spec(li, parsers[li][0]) for li in range(4)])
        assert gp.hook_counts() == want
        gp.close()
        assert h2dev.job_hook_counts(L.job) == (0, 0)
    for p, _ in parsers:
        p.close()
    L.close()


def test_unlisted_links_are_carried_as_recorded(gpu, fused):
    from grpc_rdma_amd import h2dev
    L = Links(gpu)
    listed = [0, 2]
    parsers = [L.parser(li) for li in listed]
    gp = h2dev.GroupPipe(L.job, [L.spec(li, parsers[i][0]) for i, li in enumerate(listed)])
    _check_steps(L, gp, listed, parsers, 2)
    for li in (1, 3):
        assert L.delivered(li) == L.recorded[li], li
        assert b"".join(L.recorded[li]) != L.wire[li]   # (placeholders, not the framed table)
    gp.close()
    for p, _ in parsers:
        p.close()
    L.close()


def test_refusals(gpu, monkeypatch):
    from grpc_rdma_amd import h2dev, stream as gs
    from grpc_rdma_amd._lib import GrdmaError
    monkeypatch.delenv("GRDMA_H2_PIPE_FUSED", raising=False)
    g = gpu
    # --- the batch
    p1, p2 = h2dev.Parser(False), h2dev.Parser(False)
    buf = g.DeviceBuffer(data=frame(0, 0, 1, grpc_msg(b"abc")) + bytes(64))
    table = [(0, 17)]
    with pytest.raises(GrdmaError):
        h2dev.deframe_batch([])
    with pytest.raises(GrdmaError):
        h2dev.deframe_batch([(p1, buf.ptr, table), (p2, buf.ptr, table), (p1, buf.ptr, table)])   # the same parser twice
    with pytest.raises(GrdmaError):
        h2dev.deframe_batch([(p1, 0, table)])                                                     # no arena
    lib = h2dev._bind()
    assert lib.grdma_h2_deframe_batch(None, 1) == -2
    too_many = (h2dev.H2DeframeItem * 257)()
    assert lib.grdma_h2_deframe_batch(too_many, 257) == -2
    # --- the group pipe
    L = Links(g)
    parsers = [L.parser(li) for li in range(4)]
    ps = [p for p, _ in parsers]

    def refused(specs, max_frame=16384):
        with pytest.raises(GrdmaError):
            h2dev.GroupPipe(L.job, specs, max_frame)
        assert h2dev.job_hook_counts(L.job) == (0, 0)

    refused([])
    refused([L.spec(0, ps[0]), (4, L.msgs[1], ps[1], 1, 64)])                      # a link index out of range
    refused([L.spec(0, ps[0]), L.spec(0, ps[1])])                         # a link listed twice
    refused([L.spec(0, ps[0]), L.spec(1, ps[0])])                         # a parser listed twice
    refused([(0, [], ps[0], 1, 64)])                                      # no messages
    refused([(0, [L.msgs[0][0]] * 4097, ps[0], 1, 64)])                   # more than 4096
    refused([L.spec(0, ps[0])], max_frame=0)
    refused([L.spec(0, ps[0])], max_frame=1 << 24)
    # a job that already carries another pipe's kernels; that pipe is left as it was
    single = h2dev.Pipe(L.job, L.msgs[1], ps[1], len(L.recorded[1]), 4 * len(L.lens[1]) + 256, link=1)
    before = h2dev.job_hook_counts(L.job)
    assert before == (1, 1)
    with pytest.raises(GrdmaError):
        h2dev.GroupPipe(L.job, [L.spec(0, ps[0])])
    assert h2dev.job_hook_counts(L.job) == before
    single.enqueue()
    r = single.sync()
    assert r["h2_error"] == 0 and r["framed"] == len(L.lens[1]) and b"".join(L.delivered(1)) == L.wire[1]
    # a parser whose assembler is attached to a pipe cannot go into a batch
    arena = g.DeviceBuffer(nbytes=1 << 20)
    asm = h2dev.Assembler(ps[1], arena)
    single.attach_assembler(asm)
    with pytest.raises(GrdmaError):
        h2dev.deframe_batch([(ps[1], buf.ptr, table)])
    single.close()
    asm.close()
    assert h2dev.deframe_batch([(p1, buf.ptr, table)])[0][0] == 0
    # after the refusals the job still runs unchanged
    assert h2dev.job_hook_counts(L.job) == (0, 0)
    r = L.job.run(gs.RUN_GRAPH)
    assert r.done
    for li in (0, 2, 3):
        assert L.delivered(li) == L.recorded[li]
    for p in ps + [p1, p2]:
        p.close()
    L.close()


def test_batch_equals_the_single_call_kernel(gpu):
    """Three transports in one launch, the middle one with a frame over MAX_FRAME_SIZE, against grdma_h2_deframe
    (k_h2_deframe) over the same slices on parsers of their own: the same events and errors, and the oracle's."""
    from grpc_rdma_amd import h2dev
    rng = random.Random(12)
    bad = frame(0, 0, 1, grpc_msg(b"q" * 7)) + (16385).to_bytes(3, "big") + bytes([0, 0]) + (1).to_bytes(4, "big") + bytes(100)
    wires = [_client_stream(21, [1], 4), bad, _client_stream(22, [1, 3], 5)]
    streams = [[1], [1], [1, 3]]
    lists = [_cut(w, rng, k) for w, k in zip(wires, (6, 3, 9))]
    batch_ts = [Transport(gpu, "b%d" % i, False, l, streams=s) for i, (l, s) in enumerate(zip(lists, streams))]
    single_ts = [Transport(gpu, "s%d" % i, False, l, streams=s) for i, (l, s) in enumerate(zip(lists, streams))]
    got = h2dev.deframe_batch([t.item(t.slices) for t in batch_ts])
    for i, t in enumerate(single_ts):
        parser, arena, table = t.item(t.slices)
        one = parser.deframe(arena, table)
        assert got[i] == one == t.expect(t.slices), i
    assert [e for e, _ in got] == [0, 2, 0]
    for t in batch_ts + single_ts:
        t.close()
