"""The message assembler on many links: grdma_h2_deframe_messages_batch / grdma_h2_asm_release_batch (k_h2_deframe_links,
then the six k_h2_asm_*_links kernels over a table of assemblers) and the group pipe with assemblers attached.  The
reference is the sequential model of tests/h2_asm_model.py, one per link, fed the oracle's events of that link, for
descriptors and bytes, and pyorc.H2Parser for events; every comparison is exact.  The cases are small enough for the
wave emulator (tests/test_h2_links_messages_emu.py)."""
import random

import pytest

from oracle import pyorc
from tests.h2_asm_model import AsmModel, OK, TOO_LARGE, NO_SPACE, TRUNCATED
from tests.h2_device_lib import (ERR_CAPACITY, SENTINEL, LinkAsm, Links, Transport, _check_steps, _client_stream,  # noqa: F401
                                 _eight_transports, cut_points, fused)
from tests.h2_helpers import frame, grpc_msg

pytestmark = pytest.mark.gpu

ALL = 1 << 63  # a release count above anything reported: everything


class MT:
    """a Transport of tests/h2_device_lib.py with a device assembler over an arena of its own and the model
    beside it"""

    def __init__(self, g, t, arena_bytes=1 << 20, max_msg=4 << 20, max_pending=4096):
        from grpc_rdma_amd import h2dev
        self.t, self.name = t, t.name
        self.arena = g.DeviceBuffer(data=bytes([SENTINEL]) * arena_bytes)
        self.asm = h2dev.Assembler(t.dev, self.arena, max_msg, max_pending)
        self.model = AsmModel(arena_bytes, max_msg, max_pending)

    def item(self, slices, rng=None):
        parser, ptr, table = self.t.item(slices, rng)
        return (parser, self.asm, ptr, table)

    def expect(self, slices):
        """(h2 error, events, [(descriptor, bytes)]) of one call: the oracle's parser, then the model over its events"""
        err, ev = self.t.expect(slices)
        return err, ev, self.model.call(ev, slices, err)

    def check(self, got, exp, what):
        """got = (h2 error, [Msg], events) of the device, exp = expect()'s"""
        err, ev, descs = exp
        assert got[0] == err, what
        assert got[2] == ev, what
        assert [tuple(m) for m in got[1]] == [d for d, _ in descs], what
        for m, (_, body) in zip(got[1], descs):
            if m.status == OK:
                assert self.asm.view(m) == body, (what, m)

    def close(self):
        self.asm.close()
        self.t.close()


def _run(mts, lists, order=None, rng=None, **kw):
    """one grdma_h2_deframe_messages_batch over mts in `order`; lists[i] = the slices of transport i in this call"""
    from grpc_rdma_amd import h2dev
    order = list(range(len(mts))) if order is None else order
    got = h2dev.deframe_messages_batch([mts[i].item(lists[i], rng) for i in order], want_events=True, **kw)
    res = [None] * len(mts)
    for k, i in enumerate(order):
        res[i] = got[k]
    return res


def test_batch_equals_the_model_per_transport(gpu):
    """Eight transports, each with its own parser, assembler and arena, in two calls (state is carried per assembler)
    with a release of everything in between; the same items in another order give the same per-item results."""
    from grpc_rdma_amd import h2dev
    results = {}
    for order_seed in (None, 5):
        mts = [MT(gpu, t) for t in _eight_transports(gpu, 31)]
        order = list(range(8))
        if order_seed is not None:
            random.Random(order_seed).shuffle(order)
            assert order != list(range(8))
        first = [m.t.slices[:(len(m.t.slices) + 1) // 2] for m in mts]
        second = [m.t.slices[(len(m.t.slices) + 1) // 2:] for m in mts]
        got, n_ok, with_msgs, spanning = [], 0, set(), 0
        for call, halves in enumerate((first, second)):
            res = _run(mts, halves, order, rng=random.Random(call) if order_seed is None else None)
            for i, m in enumerate(mts):
                exp = m.expect(halves[i])
                assert exp[0] == 0
                m.check(res[i], exp, (m.name, call))
                n_ok += sum(1 for d, _ in exp[2] if d[4] == OK)
                if exp[2]:
                    with_msgs.add(i)
            if call == 0:
                spanning = sum(len(m.model.carried) for m in mts)
                h2dev.release_batch([(mts[i].asm, ALL) for i in order])
                for m in mts:
                    m.model.release()
            got.append([(r[0], [tuple(x) for x in r[1]], r[2]) for r in res])
        # (the model's own output shows the case is one)
        assert n_ok >= 40 and spanning >= 1 and len(with_msgs) >= 5
        assert got[0][7] == (0, [], []) and got[1][7] == (0, [], [])  # the empty transport
        for m in mts:
            assert m.asm.stats()["bytes_in_use"] == m.model.bytes_in_use(), m.name
            assert m.t.dev.live_streams() == m.t.orc.live_streams(), m.name
            m.close()
        results[order_seed] = got
    assert results[None] == results[5]


def test_batch_equals_the_single_call(gpu):
    """Three transports through the batch and, on parsers and assemblers of their own, through
    grdma_h2_deframe_messages: the same descriptors, bytes, errors and counters."""
    rng = random.Random(12)
    bad = frame(0, 0, 1, grpc_msg(b"q" * 7)) + frame(0, 0, 1, grpc_msg(b"r" * 900)[:300]) + \
        (16385).to_bytes(3, "big") + bytes([0, 0]) + (1).to_bytes(4, "big") + bytes(100)
    wires = [_client_stream(21, [1], 4), bad, _client_stream(22, [1, 3], 5)]
    streams = [[1], [1], [1, 3]]
    lists = [cut_points(w, rng, k) for w, k in zip(wires, (6, 3, 9))]
    batch = [MT(gpu, Transport(gpu, "b%d" % i, False, l, streams=s)) for i, (l, s) in enumerate(zip(lists, streams))]
    single = [MT(gpu, Transport(gpu, "s%d" % i, False, l, streams=s)) for i, (l, s) in enumerate(zip(lists, streams))]
    got = _run(batch, lists)
    for i, (b, s) in enumerate(zip(batch, single)):
        parser, asm, arena, table = s.item(lists[i])
        err, msgs, ev = parser.deframe_messages(arena, table, asm, want_events=True)
        assert (got[i][0], [tuple(m) for m in got[i][1]], got[i][2]) == (err, [tuple(m) for m in msgs], ev), i
        assert [b.asm.view(m) for m in got[i][1] if m.status == OK] == [s.asm.view(m) for m in msgs if m.status == OK], i
        b.check(got[i], b.expect(lists[i]), i)
        sb, ss = b.asm.stats(), s.asm.stats()
        for k in ("plan_us", "copy_us"):
            sb.pop(k), ss.pop(k)
        assert sb == ss, i
    assert [r[0] != 0 for r in got] == [False, True, False]
    for m in batch + single:
        m.close()


def _trouble(g, tag):
    body = bytes(range(256)) * 40
    m = grpc_msg(body)
    whole = lambda sid, b: frame(0, 0, sid, grpc_msg(b))  # noqa: E731
    rng = random.Random(9)
    return [
        MT(g, Transport(g, "good" + tag, False, cut_points(_client_stream(3, [1, 3], 7), rng, 9), streams=[1, 3])),
        # 2 KiB of ring: the second message does not fit behind the first, nor does anything after it
        MT(g, Transport(g, "small-arena" + tag, False, [whole(1, b"x" * 1000), whole(1, b"y" * 1500), whole(1, b"z" * 10)],
                        streams=[1]), arena_bytes=2048),
        MT(g, Transport(g, "small-limit" + tag, False, [whole(1, b"a" * 50) + whole(1, b"b" * 300), whole(1, b"c" * 20)],
                        streams=[1]), max_msg=100),
        MT(g, Transport(g, "reset" + tag, False, [whole(3, b"k" * 70), frame(0, 0, 1, m[:5000]),
                                                 frame(3, 0, 1, (8).to_bytes(4, "big")), whole(3, b"l" * 7)], streams=[1, 3])),
        MT(g, Transport(g, "conn-error" + tag, False, [frame(0, 0, 7, m[:3000]),
                                                      (20000).to_bytes(3, "big") + bytes([0, 0]) + (7).to_bytes(4, "big")],
                        streams=[7])),
        MT(g, Transport(g, "small-cap" + tag, False, cut_points(_client_stream(4, [5], 5), rng, 3), streams=[5])),
    ]


def test_trouble_stays_with_its_link(gpu):
    mts = _trouble(gpu, "")
    lists = [m.t.slices for m in mts]
    got = _run(mts, lists, ev_caps=[None, None, None, None, None, 3])
    seen = set()
    for i, m in enumerate(mts):
        exp = m.expect(lists[i])
        if m.name == "small-cap":
            assert len(exp[1]) > 3 and got[i][1] == -ERR_CAPACITY and got[i][2] == -ERR_CAPACITY
            continue
        m.check(got[i], exp, m.name)
        seen |= {d[4] for d, _ in exp[2]}
    assert seen == {OK, TOO_LARGE, NO_SPACE, TRUNCATED}   # (in the MODEL's output)
    assert got[4][0] != 0 and [r[0] for r in got[:4]] == [0, 0, 0, 0]
    # the good transport alone gets what it got among the others
    alone = _trouble(gpu, "-alone")[:1]
    one = _run(alone, lists[:1])
    assert (one[0][0], [tuple(x) for x in one[0][1]], one[0][2]) == (got[0][0], [tuple(x) for x in got[0][1]], got[0][2])
    assert [alone[0].asm.view(x) for x in one[0][1]] == [mts[0].asm.view(x) for x in got[0][1]]
    for m in mts + alone:
        m.close()


def test_ring_pressure_over_many_calls(gpu):
    """Four transports, rings of a few granules more than the largest message, partial releases through the batched
    release: descriptors, offsets (wraps to 0 included) and the bytes in use equal the model after every call."""
    from grpc_rdma_amd import h2dev
    rng = random.Random(7)
    sizes = [0, 1, 255, 256, 257, 700, 1500, 3000]
    mts = [MT(gpu, Transport(gpu, "ring%d" % i, False, [], streams=[1]), arena_bytes=3072 + 256 * (2 + i), max_pending=6)
           for i in range(4)]
    wraps, no_space, sized_before = [0] * 4, [0] * 4, [False] * 4
    for call in range(14):
        lists = [[frame(0, 0, 1, grpc_msg(bytes([call * 4 + i]) * rng.choice(sizes))) for _ in range(rng.randrange(1, 5))]
                 for i in range(4)]
        got = _run(mts, lists)
        for i, m in enumerate(mts):
            exp = m.expect(lists[i])
            m.check(got[i], exp, (i, call))
            for d, _ in exp[2]:
                no_space[i] += d[4] == NO_SPACE
                if d[4] == OK and d[1]:
                    wraps[i] += sized_before[i] and d[0] == 0
                    sized_before[i] = True
        counts = [rng.randrange(0, 4) for _ in mts]
        h2dev.release_batch([(m.asm, c) for m, c in zip(mts, counts)])
        for m, c in zip(mts, counts):
            m.model.release(c)
            assert m.asm.stats()["bytes_in_use"] == m.model.bytes_in_use(), (m.name, call)
    assert all(w >= 1 for w in wraps) and all(x >= 1 for x in no_space), (wraps, no_space)
    for m in mts:
        m.close()


# ---- the group pipe with assemblers ----------------------------------------------------------------------------------
def _group_case(gpu, fused, pipeline, with_asm, steps):
    from grpc_rdma_amd import h2dev
    from grpc_rdma_amd._lib import GrdmaError
    L = Links(gpu, pipeline=pipeline)
    parsers = [L.parser(li) for li in range(4)]
    gp = h2dev.GroupPipe(L.job, [L.spec(li, parsers[li][0]) for li in range(4)])
    las = [LinkAsm(L, li, parsers[li][0]) if li in with_asm else None for li in range(4)]
    gp.attach_assemblers([la.asm if la else None for la in las])
    assert gp.hook_counts() == ((1, 7) if fused else (0, 0))   # ONE kernel in front, 1 + 6 behind, for four links
    for step in range(steps):
        _check_steps(L, gp, [0, 1, 2, 3], parsers, 1)
        for li, la in enumerate(las):
            if la:
                la.check_step(L, gp.messages(li), (step, li))
            else:
                with pytest.raises(GrdmaError):
                    gp.messages(li)
    assert len(with_asm) < 4 or any(la.closed for la in las)   # (a stream ended by its last message: later steps skip its DATA)
    gp.close()
    assert h2dev.job_hook_counts(L.job) == (0, 0)
    for la in las:
        if la:
            la.asm.close()
    for p, _ in parsers:
        p.close()
    L.close()


@pytest.mark.parametrize("pipeline", [False, True], ids=["plain", "pipelined"])
def test_group_pipe_with_assemblers(gpu, fused, pipeline):
    """Four links (2 and 3 are the two directions of one pair), five steps: after every step and per link what the
    group pipe's own test checks, the descriptors equal to the model's, the bytes in the arena equal to the bodies."""
    _group_case(gpu, fused, pipeline, {0, 1, 2, 3}, 5)


def test_group_pipe_with_assemblers_on_two_links(gpu, fused):
    """None for links 1 and 3: their events are still the oracle's, their messages are refused."""
    _group_case(gpu, fused, False, {0, 2}, 3)


def test_refusals(gpu, monkeypatch):
    from grpc_rdma_amd import h2dev
    from grpc_rdma_amd._lib import GrdmaError
    monkeypatch.delenv("GRDMA_H2_PIPE_FUSED", raising=False)
    g = gpu
    lib = h2dev.load()
    wire = frame(0, 0, 1, grpc_msg(b"abc"))
    buf = g.DeviceBuffer(data=wire + bytes(64))
    table = [(0, len(wire))]
    p1, p2 = h2dev.Parser(False), h2dev.Parser(False)
    for p in (p1, p2):
        assert p.open_streams([1]) == 0
    ar1, ar2 = g.DeviceBuffer(nbytes=1 << 16), g.DeviceBuffer(nbytes=1 << 16)
    a1, a2 = h2dev.Assembler(p1, ar1), h2dev.Assembler(p2, ar2)

    def batch_refused(items):
        with pytest.raises(GrdmaError):
            h2dev.deframe_messages_batch(items)

    # --- the batch: nothing runs
    batch_refused([])
    assert lib.grdma_h2_deframe_messages_batch(None, 1) == -2
    assert lib.grdma_h2_deframe_messages_batch((h2dev.H2MessagesItem * 257)(), 257) == -2
    batch_refused([(p1, None, buf.ptr, table)])                                    # no assembler
    batch_refused([(p1, a2, buf.ptr, table)])                                      # another parser's assembler
    batch_refused([(p1, a1, buf.ptr, table), (p2, a2, buf.ptr, table), (p1, a1, buf.ptr, table)])   # listed twice
    batch_refused([(p1, a1, 0, table)])                                            # no arena
    with pytest.raises(GrdmaError):
        h2dev.release_batch([])
    with pytest.raises(GrdmaError):
        h2dev.release_batch([(a1, 1), (a2, 1), (a1, 1)])
    assert a1.stats()["reported"] == 0 and p1.live_streams() == 1
    r = h2dev.deframe_messages_batch([(p1, a1, buf.ptr, table)])
    assert r[0][0] == 0 and [(m.length, m.status) for m in r[0][1]] == [(3, OK)] and a1.view(r[0][1][0]) == b"abc"
    h2dev.release_batch([(a1, 1)])
    assert a1.stats()["bytes_in_use"] == 0

    # --- the group pipe
    L = Links(g)
    parsers = [L.parser(li) for li in range(4)]
    ps = [p for p, _ in parsers]
    gp = h2dev.GroupPipe(L.job, [L.spec(li, ps[li]) for li in range(4)])
    las = [LinkAsm(L, li, ps[li]) for li in range(4)]
    asms = [la.asm for la in las]
    # an assembler that a single pipe (on another job) has attached
    L2 = Links(g)
    px, _ = L2.parser(1)
    single = h2dev.Pipe(L2.job, L2.msgs[1], px, len(L2.recorded[1]), 4 * len(L2.lens[1]) + 256, link=1)
    arx = g.DeviceBuffer(nbytes=1 << 20)
    ax = h2dev.Assembler(px, arx)
    single.attach_assembler(ax)
    before = gp.hook_counts()
    assert before == (1, 1)

    def attach_refused(lst):
        with pytest.raises(GrdmaError):
            gp.attach_assemblers(lst)
        assert gp.hook_counts() == before

    attach_refused(asms[:3])                                  # wrong n
    attach_refused(asms + [None])
    attach_refused([None] * 4)                                # all NULL
    attach_refused([asms[1], asms[0], None, None])            # assemblers of other parsers than their specs'
    attach_refused([a1, None, None, None])
    attach_refused([asms[0], ax, None, None])                 # attached to another pipe (and a foreign parser's)
    _check_steps(L, gp, [0, 1, 2, 3], parsers, 1)             # the pipe still steps as before, without assemblers
    with pytest.raises(GrdmaError):
        gp.messages(0)
    for la in las:                                            # (their oracle parsers follow the step)
        for s in L.delivered(la.li):
            rc, e = la.orc.feed(s)
            la.closed |= {x[3] for x in e if x[0] == pyorc.EV_STREAM_CLOSED}
    gp.attach_assemblers(asms)
    before = gp.hook_counts()
    assert before == (1, 7)
    attach_refused(asms)                                      # a second attach
    # attached assemblers are the pipe's: no release, no batch, and closing them does nothing
    with pytest.raises(GrdmaError):
        asms[0].release(1)
    with pytest.raises(GrdmaError):
        h2dev.release_batch([(a1, 0), (asms[2], 1)])
    batch_refused([(p1, a1, buf.ptr, table), (ps[0], asms[0], buf.ptr, table)])
    with pytest.raises(GrdmaError):
        h2dev.deframe_batch([(ps[3], buf.ptr, table)])
    assert gp.hook_counts() == before
    for step in range(2):
        _check_steps(L, gp, [0, 1, 2, 3], parsers, 1)
        for li, la in enumerate(las):
            la.check_step(L, gp.messages(li), (step, li))
    gp.close()
    assert h2dev.job_hook_counts(L.job) == (0, 0)
    # detached: the assembler is the caller's again
    asms[0].release(ALL)
    h2dev.release_batch([(asms[1], ALL), (asms[2], ALL)])
    single.close()
    for a in asms + [ax, a1, a2]:
        a.close()
    for p in ps + [px, p1, p2]:
        p.close()
    L.close()
    L2.close()
