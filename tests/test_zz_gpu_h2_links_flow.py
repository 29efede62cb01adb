"""Receive flow control on many links: grdma_h2_fc_account_batch (the five k_h2_links_fc_* kernels over a table of ledgers)
and the group pipe with ledgers attached.  Expected values come from the Model of tests/h2_flow_model.py -- the rules
of include/grdma_amd.h applied to the ORACLE's event list -- with struct.pack for the frames and the 23-byte cut for the
slices; nothing of the library's own events or output goes into it, and every comparison is exact.  The cases are small
enough for the wave emulator (tests/test_h2_links_flow_emu.py)."""
import random

import pytest

from oracle import pyorc
from tests.h2_device_lib import (FH, FLOW_SIZES as SIZES, Echo, LinkAsm, Links, _check_steps, _interleaved,  # noqa: F401
                                 _pipe_setup, _server_call, fused, oracle_parser, pack_slices, read_slices, step_events)
from tests.h2_flow_model import CONN, LOST, STREAM, Model
from tests.h2_helpers import frame, grpc_msg

pytestmark = pytest.mark.gpu

H2FC_ONE_THREADS = 512   # csrc/grdma_h2_fc.h
WRAP8 = (29, 31, 33, 61, 63, 65, 93, 95)   # at 16 slots: homes 14 15 0 14 15 0 14 15
assert [(s >> 1) & 15 for s in WRAP8] == [14, 15, 0, 14, 15, 0, 14, 15]


# ---- the batch call --------------------------------------------------------------------------------------------------
def _expect(h, cap=None, hdr_cap=None, lost=False):
    """the model over the oracle's events of h's last deframing -> (slice lengths, result tuple, wire)"""
    cap = h.cap if cap is None else cap
    hdr_cap = 32 * cap if hdr_cap is None else hdr_cap
    if lost:
        return h.model.lost_call()
    err_o, ev_o = h.oracle()
    return h.model.call(ev_o, err_o, cap, hdr_cap)


def _batch(g, hs, order, lost=()):
    """one grdma_h2_fc_account_batch over the harnesses hs, listed in `order`; every item against its model"""
    from grpc_rdma_amd import h2dev
    for h in hs:
        h.new_target()
    got = h2dev.account_batch([(hs[i].fc, hs[i].slices.ptr, hs[i].cap, hs[i].hdr.ptr, 32 * hs[i].cap) for i in order])
    assert len(got) == len(order)
    out = [None] * len(hs)
    for k, i in enumerate(order):
        h = hs[i]
        lens, res, wire = _expect(h, lost=i in lost)
        print("ledger %d: %r -> %r" % (i, res, got[k]))
        if res[7]:
            assert got[k] == (res, None), i
        h.check_accounted((lens, res, wire), None if res[7] else got[k], "ledger %d" % i)
        out[i] = (res, wire)
    return out


NINE = [
    dict(streams=(1, 3, 5), stream_window=1 << 20, conn_window=1 << 24),                         # 0 a client side
    dict(prefix=True, stream_window=1 << 20, conn_window=1 << 22),                               # 1 a server side
    dict(streams=(1,)),                                                                          # 2 a call without DATA
    dict(streams=(1,)),                                                                          # 3 zero events
    dict(streams=WRAP8, stream_window=1 << 20, conn_window=1 << 20, table_slots=16),             # 4 a small table
    dict(streams=(1, 3), stream_window=1 << 20, conn_window=1 << 20, max_updates=3),             # 5 few updates
    dict(streams=(1, 3, 5), stream_window=1 << 20, conn_window=200000, conn_threshold=100000),   # 6 a threshold
    dict(streams=(1, 3), stream_window=20000, conn_window=1 << 20),                              # 7 a small stream window
    dict(streams=(7,), stream_window=1 << 20, conn_window=65535, conn_threshold=65535, max_updates=4096),   # 8
]


def _nine_calls(call):
    whole = frame(0, 0, 3, grpc_msg(b"z" * 5000))
    return [
        _interleaved(call, (1, 3, 5), SIZES if call == 0 else SIZES[:5]),
        _server_call() if call == 0 else [frame(1, 4, 7, b"\x82"), whole[:2000], frame(0, 0, 1, b"late" * 10)],
        [frame(6, 0, 0, bytes(8))],
        [],
        _interleaved(call + 3, WRAP8, [40, 0, 900, 16384, 7, 300, 2, 5000, 1, 60, 16384, 33, 4, 800, 9, 10]),
        [frame(0, 0, 3, b"a" * 100), frame(0, 0, 1, b"b" * 5000), frame(0, 0, 3, b"c" * 7)],
        _interleaved(call + 1, (1, 3, 5), SIZES),
        [frame(0, 0, 3, b"a" * 100), frame(0, 0, 1, b"b" * 16384), frame(0, 0, 1, b"c" * (16384 if call == 0 else 10))],
        [frame(0, 0, 7, b"a" * 16384)] * (3 - call),
    ]


def _nine(g):
    return [FH(g, **kw) for kw in NINE]


def test_batch_equals_the_model_per_transport(gpu):
    """Nine ledgers in one call, listed in shuffled order, two calls in a row: `announced` carries over per link."""
    hs = _nine(gpu)
    order = list(range(9))
    random.Random(4).shuffle(order)
    assert order != list(range(9))
    outs = []
    for call in (0, 1):
        for h, slices in zip(hs, _nine_calls(call)):
            h.deframe_checked(slices)
        outs.append(_batch(gpu, hs, order))
    first, second = outs
    assert hs[0].model.frames[0][0] == 0 and sorted(s for s, _ in hs[0].model.frames) == [0, 1, 3, 5]
    assert first[1][0][0] == 2 and first[1][0][3] == 105 + 3005 + 55 + 4000 + 10 + 700   # the connection's and stream 3's
    assert first[2][0][:3] == (0, 0, 0) and first[3][0] == (0, 0, 0, 0, 0, 0, 0, 0) == second[3][0]
    assert first[4][0][0] == 9 and first[5][0][0] == 3 and first[5][0][7] == 0
    # the threshold: no connection frame in the first call, the credit of both in the second
    assert first[6][0][0] == 3 and second[6][0][0] == 4 and hs[6].model.frames[0] == (0, 2 * sum(SIZES))
    assert first[7][0][5] == STREAM and first[7][0][6] == 1 and second[7][0][5] == 0
    assert first[8][0][5] == 0 and second[8][0][5] == CONN and hs[8].model.frames[0] == (0, 5 * 16384)
    for h in hs:
        h.close()


def test_batch_equals_the_single_call(gpu):
    """The same deframings accounted once by account_batch and once, on twin parsers, by FlowControl.account."""
    batch, single = _nine(gpu), _nine(gpu)
    for call in (0, 1):
        calls = _nine_calls(call)
        for hb, hs_, slices in zip(batch, single, calls):
            assert hb.deframe(slices) == hs_.deframe(slices)
        _batch(gpu, batch, list(range(9)))
        for i, (hb, h1) in enumerate(zip(batch, single)):
            h1.new_target()
            sl, res, wire = h1.fc.account(h1.slices.ptr, h1.cap, h1.hdr.ptr, 32 * h1.cap)
            assert res == hb.fc.last_result, (call, i)
            # slice tables (the pointers relative to each header arena), header arena bytes, counters
            n = res[1]
            tb, t1 = read_slices(gpu, hb.slices, n), read_slices(gpu, h1.slices, n)
            assert [(p - hb.hdr.ptr, ln) for p, ln in tb] == [(p - h1.hdr.ptr, ln) for p, ln in t1] == \
                [(32 * k, ln) for k, (_, ln) in enumerate(sl)], (call, i)
            assert hb.slices.read()[16 * n:] == h1.slices.read()[16 * n:]
            assert hb.hdr.read() == h1.hdr.read(), (call, i)
            sb, s1 = hb.fc.stats(), h1.fc.stats()
            sb.pop("kernel_us"), s1.pop("kernel_us")
            assert sb == s1, (call, i)
    for h in batch + single:
        h.close()


def test_trouble_stays_with_its_link(gpu):
    four = [frame(0, 0, s, b"a" * 10) for s in (1, 3, 5, 7)]
    hs = [FH(gpu, streams=(1,), stream_window=1 << 20, conn_window=1 << 20),                       # 0 event overflow
          FH(gpu, streams=(1, 3), stream_window=1 << 20, conn_window=1 << 20),                     # 1 connection error
          FH(gpu, streams=(1, 3, 5, 7), stream_window=1 << 20, conn_window=1 << 20, max_updates=4, cap=8),   # 2 too many frames
          FH(gpu, streams=(1, 3), stream_window=20000, conn_window=65535),                         # 3 both windows broken
          FH(gpu, streams=(1, 3, 5), stream_window=1 << 20, conn_window=1 << 24)]                  # 4 nothing wrong
    with pytest.raises(gpu.GrdmaError, match="error 5"):
        hs[0].deframe([frame(0, 0, 1, b"b" * 10)] * 40, ev_cap=16)
    err, _ = hs[1].deframe_checked([frame(0, 0, 1, b"a" * 500), frame(0, 0, 3, b"b" * 70), frame(6, 0, 0, b"short"),
                                      frame(0, 0, 1, b"never parsed")])
    assert err == 15
    hs[2].deframe_checked(four)
    hs[3].deframe_checked([frame(0, 0, 3, b"c" * 100)] + [frame(0, 0, 1, b"a" * 16384)] * 5)
    hs[4].deframe_checked(_interleaved(0, (1, 3, 5), SIZES))
    out = _batch(gpu, hs, [3, 0, 4, 2, 1], lost={0})
    assert out[0][0] == (0, 0, 0, 0, 0, LOST, 0, 2)
    assert out[1][0] == (0, 0, 0, 570, 0, 0, 0, 0)
    assert out[2][0][7] == 1 and out[2][0][0] == 5
    assert out[3][0][5] == CONN | STREAM and out[3][0][6] == 1 and out[3][0][7] == 0
    assert out[4][0][0] == 4 and out[4][0][5] == 0 and out[4][0][7] == 0
    # a second call: the lost flag is sticky on its link alone, the cap overflow is gone, the others go on
    for h, slices in zip(hs, ([frame(0, 0, 1, b"d" * 9)], None, four[:2], [frame(0, 0, 3, b"e" * 50)], _interleaved(1, (1, 3, 5), SIZES[:5]))):
        if slices is not None:
            h.deframe_checked(slices)
    ok = [0, 2, 3, 4]   # (the dead connection has deframed nothing new: it stays out)
    sub = [hs[i] for i in ok]
    out = _batch(gpu, sub, [2, 1, 3, 0])
    assert out[0][0][5] == LOST and out[0][0][7] == 0 and out[0][0][0] == 2
    assert out[1][0][7] == 0 and out[1][0][0] == 3
    assert out[2][0][5] == 0 and out[3][0][5] == 0
    for h in hs:
        h.close()


def _small_frames(rng, ids, nframes):
    """nframes DATA frames with one small gRPC message each, the streams interleaved at random, twenty to a slice"""
    frames = [frame(0, 0, rng.choice(ids), grpc_msg(bytes(rng.randrange(0, 40)))) for _ in range(nframes)]
    return [b"".join(frames[i:i + 20]) for i in range(0, len(frames), 20)]


def _three(gpu, middle_kw, slices, more_than):
    three = [frame(0, 0, 1, b"a" * 10), frame(0, 0, 3, b"b" * 20), frame(0, 0, 1, b"c" * 30)]
    hs = [FH(gpu, streams=(1, 3), stream_window=1 << 20, conn_window=1 << 20), FH(gpu, **middle_kw),
          FH(gpu, streams=(1, 3), stream_window=1 << 20, conn_window=1 << 20)]
    hs[0].deframe_checked(three)
    _, ev = hs[1].deframe_checked(slices, ev_cap=1 << 16)
    hs[2].deframe_checked(three)
    assert len(hs[1].oracle()[1]) > more_than and len(ev) > more_than
    out = _batch(gpu, hs, [0, 1, 2])
    assert out[0] == out[2] and out[0][0][0] == 3 and out[0][0][3] == 60
    return hs, out


def test_grid_stride_inside_a_share(gpu):
    """More than 8 * 256 events on eight colliding stream ids at 16 slots, between two three-frame links."""
    rng = random.Random(41)
    hs, out = _three(gpu, dict(streams=WRAP8, stream_window=1 << 20, conn_window=1 << 24, table_slots=16),
                     _small_frames(rng, WRAP8, 900), 8 * 256)
    assert out[1][0][0] == 9 and out[1][0][5] == 0 and out[1][0][7] == 0 and out[1][0][3] == out[1][0][4]
    # (the scratch table is cleared between calls)
    hs[1].deframe_checked(_small_frames(rng, WRAP8, 60))
    assert _batch(gpu, hs[1:2], [0])[0][0][0] == 9
    for h in hs:
        h.close()


def test_finish_scan_past_one_block(gpu):
    """One link's event list is longer than 32 * H2FC_ONE_THREADS: the finish's scan over mark words takes a second block."""
    rng = random.Random(42)
    ids = (1, 3, 5, 7, 9)
    slices = _small_frames(rng, ids[:4], 5200) + [frame(0, 0, 9, grpc_msg(b"last"))]   # (a first frame behind word 512)
    hs, out = _three(gpu, dict(streams=ids, stream_window=1 << 20, conn_window=1 << 24), slices, 32 * H2FC_ONE_THREADS)
    assert out[1][0][0] == 6 and out[1][0][7] == 0 and hs[1].model.frames[-1] == (9, 9)
    for h in hs:
        h.close()


# ---- the group pipe with ledgers ----------------------------------------------------------------------------------
LEDGERS = [dict(stream_window=1 << 20, conn_window=1 << 22, conn_threshold=0, max_updates=16),
           dict(stream_window=1 << 20, conn_window=1 << 22, conn_threshold=150000, max_updates=4),
           dict(stream_window=100000, conn_window=1 << 22, conn_threshold=0, max_updates=16),    # stream 9 sends 200000
           dict(stream_window=1 << 20, conn_window=1 << 23, conn_threshold=0, max_updates=64)]


class LinkLedger:
    """per listed link: a device ledger, the model and an oracle parser of its own (the events the model is fed)"""

    def __init__(self, L, li, parser):
        from grpc_rdma_amd import h2dev
        self.li, kw = li, LEDGERS[li]
        sids = L.streams(li)
        self.fc = h2dev.FlowControl(parser, **kw)
        self.model = Model(kw["stream_window"], kw["conn_window"], kw["conn_threshold"], kw["max_updates"], sids)
        self.cap = (13 * kw["max_updates"] + 22) // 23
        self.orc = oracle_parser(False, L.max_frame, sids)

    def check_step(self, L, got, what):
        """got = the group pipe's window_updates of this link for the step that just ended"""
        ev = step_events(self.orc, L.delivered(self.li), what)
        lens, res, wire = self.model.call(ev, 0, self.cap, 32 * self.cap)
        sl, r, w = got
        print("link %d step %r: %r -> %r" % (self.li, what, res, r))
        assert r == res and [n for _, n in sl] == lens and w == wire, what
        assert res[7] == 0
        return ev


def _group_run(gpu, fused, with_fc, with_asm, asm_first, steps):
    """-> per step and link (events, messages or None); with ledgers every step's window updates against the model"""
    from grpc_rdma_amd import h2dev
    from grpc_rdma_amd._lib import GrdmaError
    L = Links(gpu)
    parsers = [L.parser(li) for li in range(4)]
    gp = h2dev.GroupPipe(L.job, [L.spec(li, parsers[li][0]) for li in range(4)])
    # (the pipe refuses a parser that has a ledger when it is created: the ledgers come behind it)
    lls = [LinkLedger(L, li, parsers[li][0]) if li in with_fc else None for li in range(4)]
    las = [LinkAsm(L, li, parsers[li][0]) if with_asm else None for li in range(4)]

    def attach_fc():
        if with_fc:
            gp.attach_flow_control([ll.fc if ll else None for ll in lls])

    def attach_asm():
        if with_asm:
            gp.attach_assemblers([la.asm for la in las])

    for attach in ((attach_asm, attach_fc) if asm_first else (attach_fc, attach_asm)):
        attach()
    behind = 1 + (5 if with_fc else 0) + (6 if with_asm else 0)
    assert gp.hook_counts() == ((1, behind) if fused else (0, 0))
    out, closed, conn_frames = [], [set() for _ in range(4)], [0] * 4
    for step in range(steps):
        _check_steps(L, gp, [0, 1, 2, 3], parsers, 1)
        row = []
        for li in range(4):
            msgs = None
            if las[li]:
                msgs = gp.messages(li)
                las[li].check_step(L, msgs, (step, li))
                msgs = [tuple(m) for m in msgs]
            row.append((gp.events(li), msgs))
            if lls[li]:
                ev = lls[li].check_step(L, gp.window_updates(li), (step, li))
                frames = lls[li].model.frames
                # a stream that closed in this step or before gets no frame: its bytes are the connection's
                closed[li] |= {e[3] for e in ev if e[0] == pyorc.EV_STREAM_CLOSED}
                assert not closed[li] & {s for s, _ in frames}, (step, li)
                conn_frames[li] += 1 if frames and frames[0][0] == 0 else 0
            elif with_fc:
                with pytest.raises(GrdmaError):
                    gp.window_updates(li)
        out.append(row)
    if 1 in with_fc:
        # (the threshold holds the connection's frame back until two steps are owed)
        assert conn_frames[1] == steps // 2 and lls[1].model.stats["frames"] == steps + steps // 2
    if 3 in with_fc:
        # link 3's stream 2 ends with the last message of the first step: from then on its bytes are the connection's
        assert closed[3] == {2} and {s for s, _ in lls[3].model.frames} == {0, 4}
    if 2 in with_fc:
        assert lls[2].model.stats["stream_overflows"] >= 1
    for ll in lls:
        if ll:
            st = ll.fc.stats()
            assert {k: st[k] for k in ll.model.stats} == ll.model.stats and st["announced"] == ll.model.announced
            ll.fc.close()   # does nothing while attached
            assert ll.fc.h
    gp.close()
    assert h2dev.job_hook_counts(L.job) == (0, 0)
    for ll in lls:
        if ll:
            ll.fc.close()
            assert ll.fc.h is None
    for la in las:
        if la:
            la.asm.close()
    for p, _ in parsers:
        p.close()
    L.close()
    return out


def test_group_pipe_with_ledgers(gpu, fused):
    """Four links (2 and 3 are the two directions of one pair), five steps, ledgers on all four: after every step and
    per link the window updates equal the model fed with that link's delivered slices; the events equal those of the same
    pipe without ledgers."""
    with_fc = _group_run(gpu, fused, {0, 1, 2, 3}, False, False, 5)
    without = _group_run(gpu, fused, set(), False, False, 5)
    assert with_fc == without


def test_group_pipe_with_ledgers_on_two_links(gpu, fused):
    """None for links 1 and 3: their events are still the oracle's, their window updates are refused."""
    _group_run(gpu, fused, {0, 2}, False, False, 3)


@pytest.mark.parametrize("asm_first", [True, False], ids=["assemblers-first", "ledgers-first"])
def test_group_pipe_with_ledgers_and_assemblers(gpu, fused, asm_first):
    """The assemblers' six kernels and the ledgers' five in either attach order: events and messages equal the same pipe
    without ledgers."""
    with_fc = _group_run(gpu, fused, {0, 1, 2, 3}, True, asm_first, 3)
    without = _group_run(gpu, fused, set(), True, True, 3)
    assert with_fc == without and all(m is not None for row in with_fc for _, m in row)


def test_refusals_and_lifetime(gpu, monkeypatch):
    from grpc_rdma_amd import h2dev, stream as gs
    from grpc_rdma_amd._lib import GrdmaError
    monkeypatch.delenv("GRDMA_H2_PIPE_FUSED", raising=False)
    g = gpu
    t = g.DeviceBuffer(nbytes=4096)
    data, table = pack_slices([frame(0, 0, 1, b"abc")])
    buf = g.DeviceBuffer(data=data)
    lib = h2dev.load()

    # --- the batch call
    def item(fc, k=0):
        return (fc, t.ptr + 1024 * k, 4, t.ptr + 1024 * k + 256, 128)

    def batch_refused(items, match):
        with pytest.raises(GrdmaError, match=match):
            h2dev.account_batch(items)

    p1, p2, p3 = h2dev.Parser(False), h2dev.Parser(False), h2dev.Parser(False)
    f1, f2, f3 = h2dev.FlowControl(p1), h2dev.FlowControl(p2), h2dev.FlowControl(p3)
    batch_refused([], "1 .. GRDMA_H2_BATCH_MAX")
    out = (h2dev.u64 * (8 * 257))()
    assert lib.grdma_h2_fc_account_batch((h2dev.H2FcItem * 257)(), 257, out) == -2
    assert lib.grdma_h2_fc_account_batch(None, 1, out) == -2
    batch_refused([item(None)], "without ledger")
    batch_refused([item(f1)], "deframed nothing yet")
    for p in (p1, p2):
        p.deframe(buf.ptr, table)
    batch_refused([item(f1), item(f2, 1), item(f1, 2)], "twice")
    batch_refused([item(f1), item(f3, 1)], "deframed nothing yet")
    batch_refused([(f1, t.ptr + 8, 4, t.ptr + 256, 128)], "misaligned")
    batch_refused([(f1, t.ptr, 0, t.ptr + 256, 128)], "misaligned")
    batch_refused([(f1, t.ptr, 4, 0, 128)], "misaligned")
    batch_refused([(f1, t.ptr, 4, t.ptr + 256, 0)], "misaligned")
    assert f1.stats()["calls"] == 0 and f2.stats()["calls"] == 0   # (nothing ran)
    got = h2dev.account_batch([item(f1), item(f2, 1)])
    assert [r[1][:4] for r in got] == [(1, 1, 13, 3)] * 2
    batch_refused([item(f1), item(f2, 1)], "accounted already")
    p2.deframe(buf.ptr, table)
    batch_refused([item(f1), item(f2, 1)], "accounted already")    # (one stale item refuses the whole call)
    assert f2.stats()["calls"] == 1
    p3.close()
    batch_refused([item(f3)], "parser is gone")
    f3.close()
    assert f3.h is None

    # --- the group pipe
    L = Links(g)
    parsers = [L.parser(li) for li in range(4)]
    ps = [p for p, _ in parsers]
    gp = h2dev.GroupPipe(L.job, [L.spec(li, ps[li]) for li in range(4)])
    fcs = [h2dev.FlowControl(p) for p in ps]
    before = gp.hook_counts()
    assert before == (1, 1)

    def attach_refused(lst, match):
        with pytest.raises(GrdmaError, match=match):
            gp.attach_flow_control(lst)
        assert gp.hook_counts() == before

    attach_refused(fcs[:3], "per link spec")                         # wrong n
    attach_refused(fcs + [None], "per link spec")
    attach_refused([None] * 4, "no ledger")                          # all NULL
    attach_refused([fcs[1], fcs[0], None, None], "another parser")   # ledgers of other parsers than their specs'
    attach_refused([f1, None, None, None], "another parser")
    attach_refused([fcs[0], None, fcs[0], None], "twice")
    # a ledger attached to a single pipe elsewhere
    px = h2dev.Parser(False)
    assert px.open_streams([1]) == 0
    (single,), (jobx,), keep = _pipe_setup(g, h2dev, gs, [100, 5000], 1, px)
    fx = h2dev.FlowControl(px)
    single.attach_flow_control(fx)
    attach_refused([fcs[0], fx, None, None], "attached to a pipe")
    batch_refused([item(fx), item(f1, 1)], "attached to a pipe")
    # a ledger whose parser is gone
    pg = h2dev.Parser(False)
    fg = h2dev.FlowControl(pg)
    pg.close()
    attach_refused([fcs[0], fg, None, None], "parser is gone")
    fg.close()
    # the attach, then: a second one; the single calls and the single pipe refuse a ledger of the group pipe
    gp.attach_flow_control([fcs[0], None, fcs[2], fcs[3]])
    before = gp.hook_counts()
    assert before == (1, 6)
    attach_refused([None, fcs[1], None, None], "attached already")
    with pytest.raises(GrdmaError, match="attached to a pipe"):
        fcs[0].account(t.ptr, 4, t.ptr + 256, 128)
    batch_refused([item(fcs[0]), item(f1, 1)], "attached to a pipe")
    lib.grdma_h2_fc_destroy(fcs[2].h)   # (does nothing while the ledger is attached: the step below runs on it)
    single.close()
    fx.close()
    assert fx.h is None
    single = h2dev.Pipe(jobx, [(keep[0][0].ptr, 100, 1, 0)], ps[0], len(jobx.delivered_slices(0)), 256)
    with pytest.raises(GrdmaError, match="another pipe"):
        single.attach_flow_control(fcs[0])
    single.close()
    jobx.close()
    px.close()
    # the refused calls left the pipe working
    gp.enqueue()
    assert all(r["h2_error"] == 0 for r in gp.sync())
    assert gp.window_updates(0)[1][7] == 0
    with pytest.raises(GrdmaError):
        gp.window_updates(1)
    for f in fcs:
        f.close()
    assert fcs[0].h and fcs[2].h and fcs[3].h and fcs[1].h is None   # close does nothing while attached
    gp.close()
    assert h2dev.job_hook_counts(L.job) == (0, 0)
    for f in fcs:
        f.close()
        assert f.h is None
    for f in (f1, f2):
        f.close()
    for p in ps + [p1, p2]:
        p.close()
    L.close()

    # --- a group reply pipe carries no ledgers (as the single reply pipe: not built)
    E = Echo(g)
    E.rp = h2dev.GroupPipe.reply(E.B.job, E.rspecs)
    fb = h2dev.FlowControl(E.parsers_back[1])
    before = h2dev.job_hook_counts(E.B.job)
    with pytest.raises(GrdmaError, match="not built"):
        E.rp.attach_flow_control([None, fb, None, None])
    assert h2dev.job_hook_counts(E.B.job) == before
    fb.close()
    assert fb.h is None   # (never attached: free to go)
    E.close()
