"""Receive flow control on the device: the window ledger (grdma_h2_fc, csrc/grdma_h2_fc.h).
The expected values come from the Model of tests/h2_flow_model.py: the rules of include/grdma_amd.h applied to the
ORACLE's event list (oracle/pyorc.H2Parser.feed), struct.pack for the frames and the 23-byte cut for the slices.
Nothing of the library's own events or output goes into the model; every comparison is exact (FH of
tests/h2_device_lib.py runs a call on the device and in the model and compares)."""
import os
import struct

import pytest

from oracle import pyorc
from oracle.pyorc import EV_FRAME, EV_STREAM_CLOSED, EV_STREAM_OPEN
from tests.h2_device_lib import (FH, FLOW_SIZES as SIZES, Echo, _back_job, _interleaved, _pipe_setup, _server_call,
                                 fast_sender_slices, pack_slices)
from tests.h2_flow_model import CONN, LOST, STREAM, Model
from tests.h2_helpers import frame, grpc_msg

pytestmark = pytest.mark.gpu


def test_client_side_windows_never_binding(gpu):
    h = FH(gpu, streams=(1, 3, 5), stream_window=1 << 20, conn_window=1 << 24, conn_threshold=0)
    res, wire = h.feed(_interleaved(0, (1, 3, 5), SIZES))
    assert res[0] == 4 and res[5] == 0 and res[3] == res[4] == sum(SIZES)
    assert [s for s, _ in h.model.frames] == [0, 1, 3, 5]
    res, _ = h.feed(_interleaved(1, (1, 3, 5), SIZES[:5]))
    assert res[0] == 4 and h.model.announced == 1 << 24
    res, _ = h.feed([frame(6, 0, 0, bytes(8))])  # (a call without DATA: nothing to return)
    assert res[:3] == (0, 0, 0)
    h.close()


def test_client_side_threshold_zero_and_half(gpu):
    h = FH(gpu, streams=(1, 3, 5), stream_window=1 << 20, conn_window=200000, conn_threshold=0)
    for seed in range(3):
        res, _ = h.feed(_interleaved(seed, (1, 3, 5), SIZES))
        assert h.model.frames[0] == (0, sum(SIZES))
    h.close()
    # half the window: calls without a connection frame, then one that carries the accumulated credit
    h = FH(gpu, streams=(1, 3, 5), stream_window=1 << 20, conn_window=200000, conn_threshold=100000)
    conn = []
    for seed in range(4):
        res, _ = h.feed(_interleaved(seed, (1, 3, 5), SIZES))
        conn.append([inc for s, inc in h.model.frames if s == 0])
    assert conn == [[], [2 * sum(SIZES)], [], [2 * sum(SIZES)]] and sum(SIZES) < 100000 <= 2 * sum(SIZES)
    h.close()


def test_server_side(gpu):
    h = FH(gpu, prefix=True, stream_window=1 << 20, conn_window=1 << 22, conn_threshold=0)
    res, _ = h.feed(_server_call())
    assert h.model.frames == [(0, 105 + 3005 + 55 + 4000 + 10 + 700), (3, 3005)]
    # a DATA frame whose payload is split across two calls counts once, in the first
    whole = frame(0, 0, 3, grpc_msg(b"z" * 5000))
    res, _ = h.feed([frame(1, 4, 7, b"\x82"), whole[:2000]])
    assert h.model.frames == [(0, 5005), (3, 5005)]
    res, _ = h.feed([whole[2000:], frame(0, 0, 7, grpc_msg(b"k" * 20))])
    assert h.model.frames == [(0, 25), (7, 25)]
    # the stream whose reads closed stays skipped in later calls (it is in the map until its writes close)
    res, _ = h.feed([frame(0, 0, 1, b"late" * 10), frame(0, 0, 7, grpc_msg(b"m"))])
    assert h.model.frames == [(0, 46), (7, 6)]
    h.close()


def test_violations(gpu):
    # one stream sends more than stream_window
    h = FH(gpu, streams=(1, 3), stream_window=20000, conn_window=1 << 20)
    res, _ = h.feed([frame(0, 0, 3, b"a" * 100), frame(0, 0, 1, b"b" * 16384), frame(0, 0, 1, b"c" * 16384)])
    assert res[5] == STREAM and res[6] == 1 and h.model.stats["stream_overflows"] == 1
    h.close()
    # a call sums to more than the announced connection window
    h = FH(gpu, streams=(1,), stream_window=1 << 20, conn_window=65535, conn_threshold=65535)
    res, _ = h.feed([frame(0, 0, 1, b"a" * 16384)] * 3)
    assert res[5] == 0 and res[0] == 1 and h.model.announced == 65535 - 3 * 16384
    res, _ = h.feed([frame(0, 0, 1, b"a" * 16384)] * 2)
    assert res[5] == CONN and h.model.frames[0] == (0, 5 * 16384) and h.model.announced == 65535
    h.close()


def test_event_overflow_is_lost(gpu):
    h = FH(gpu, streams=(1,), stream_window=1 << 20, conn_window=1 << 20)
    h.feed([frame(0, 0, 1, b"a" * 100)])
    with pytest.raises(gpu.GrdmaError, match="error 5"):
        h.deframe([frame(0, 0, 1, b"b" * 10)] * 40, ev_cap=16)
    h.model.lost_call()
    with pytest.raises(gpu.GrdmaError, match="error 5"):
        h.fc.account(h.slices.ptr, h.cap, h.hdr.ptr, 32 * h.cap)
    assert h.fc.last_result == (0, 0, 0, 0, 0, LOST, 0, 2)
    h.check_stats()  # (the flag, nothing else)
    h.close()


def test_connection_error_counts_and_emits_nothing(gpu):
    h = FH(gpu, streams=(1, 3), stream_window=1 << 20, conn_window=1 << 20)
    err, ev = h.deframe([frame(0, 0, 1, b"a" * 500), frame(0, 0, 3, b"b" * 70), frame(6, 0, 0, b"short"),
                         frame(0, 0, 1, b"never parsed")])
    assert err == 15
    res, wire = h.account()
    assert res == (0, 0, 0, 570, 0, 0, 0, 0) and wire == b"" and h.model.announced == (1 << 20) - 570
    h.close()


def test_capacity_overflows(gpu):
    call = [frame(0, 0, s, b"a" * 10) for s in (1, 3, 5, 7)]
    # more frames than max_updates
    h = FH(gpu, streams=(1, 3, 5, 7), stream_window=1 << 20, conn_window=1 << 20, max_updates=4, cap=8)
    res, _ = h.feed(call)
    assert res[7] == 1 and res[0] == 5 and h.model.announced == 1 << 20  # (the window state advanced)
    res, _ = h.feed(call[:2])
    assert res[7] == 0 and res[0] == 3
    h.close()
    # a slice cap, then a header cap too small
    h = FH(gpu, streams=(1, 3, 5, 7), stream_window=1 << 20, conn_window=1 << 20, max_updates=16, cap=8)
    res, _ = h.feed(call, cap=2)
    assert res[7] == 1 and res[1] == 3
    res, _ = h.feed(call, cap=3, hdr_cap=64)
    assert res[7] == 1
    res, _ = h.feed(call, cap=3)
    assert res[7] == 0 and res[1] == 3
    h.close()


def test_round_trip(gpu):
    from grpc_rdma_amd import h2dev
    h = FH(gpu, streams=(1, 3, 5), stream_window=1 << 20, conn_window=1 << 20)
    _, wire = h.feed(_interleaved(2, (1, 3, 5), SIZES))
    want = [s for s, _ in h.model.frames]
    assert len(want) == 4 and len(wire) == 52
    orc = pyorc.H2Parser(False)
    for s in (1, 3, 5):
        assert orc.open_stream(s) == 0
    rc, ev = orc.feed(wire)
    assert rc == 0 and [(e[1], e[3], e[4]) for e in ev if e[0] == EV_FRAME] == [(8, s, 4) for s in want]
    back = h2dev.Parser(False)
    assert back.open_streams([1, 3, 5]) == 0
    data, table = pack_slices([wire[:23], wire[23:46], wire[46:]])
    buf = gpu.DeviceBuffer(data=data)
    err, ev = back.deframe(buf.ptr, table)
    assert err == 0 and [(e[1], e[3], e[4]) for e in ev if e[0] == EV_FRAME] == [(8, s, 4) for s in want]
    # the check looks at our bytes and not past them: a frame of length 5 is refused
    bad = struct.pack(">BHBBII", 0, 5, 8, 0, 1, 100)
    data, table = pack_slices([bad])
    buf = gpu.DeviceBuffer(data=data)
    err, _ = back.deframe(buf.ptr, table)
    assert err == 16
    back.close()
    h.close()


def test_with_the_assembler(gpu):
    from grpc_rdma_amd import h2dev
    slices = [frame(0, 0, 1, grpc_msg(b"a" * 3000)), frame(0, 0, 3, grpc_msg(b"b" * 10)), frame(0, 0, 1, grpc_msg(b""))]
    data, table = pack_slices(slices)
    buf = gpu.DeviceBuffer(data=data)
    runs = []
    for with_ledger in (False, True):
        h = FH(gpu, streams=(1, 3), stream_window=1 << 20, conn_window=1 << 20) if with_ledger else None
        parser = h.parser if h else h2dev.Parser(False)
        if not h:
            assert parser.open_streams([1, 3]) == 0
        arena = gpu.DeviceBuffer(nbytes=1 << 16)
        a = h2dev.Assembler(parser, arena, 4 << 20, 64)
        err, msgs, ev = parser.deframe_messages(buf.ptr, table, a, want_events=True)
        runs.append((err, [tuple(m) for m in msgs], ev))
        if h:
            h.told(slices)
            res, _ = h.account()
            assert res[0] == 3 and res[3] == 3005 + 15 + 5
            with pytest.raises(gpu.GrdmaError, match="accounted already"):
                h.fc.account(h.slices.ptr, h.cap, h.hdr.ptr, 32 * h.cap)
        a.close()
        if h:
            h.close()
        else:
            parser.close()
    assert runs[0] == runs[1] and len(runs[0][1]) == 3


@pytest.mark.parametrize("fused", ["1", "0"])
def test_in_a_pipe(gpu, fused):
    g = gpu
    from grpc_rdma_amd import h2dev, stream as gs
    sizes = [70000, 1, 16379, 0, 20000, 5000]
    bodies = [bytes((j * 7 + i) % 251 for j in range(n)) for i, n in enumerate(sizes)]
    wire, _ = pyorc.h2_frame_batch(bodies, [1] * len(sizes), [0] * len(sizes), 16384)
    orc = pyorc.H2Parser(False)
    assert orc.open_stream(1) == 0
    old = os.environ.get("GRDMA_H2_PIPE_FUSED")
    os.environ["GRDMA_H2_PIPE_FUSED"] = fused
    runs = []
    try:
        for with_ledger in (False, True):
            parser = h2dev.Parser(False)
            assert parser.open_streams([1]) == 0
            (pipe,), (job,), keep = _pipe_setup(g, h2dev, gs, sizes, 1, parser)
            arena = g.DeviceBuffer(nbytes=512 << 10)
            a = h2dev.Assembler(parser, arena, 4 << 20, 4096)
            before = h2dev.job_hook_counts(job)
            pipe.attach_assembler(a)
            fc = model = None
            if with_ledger:
                fc = h2dev.FlowControl(parser, stream_window=1 << 20, conn_window=1 << 20, conn_threshold=200000, max_updates=16)
                model = Model(1 << 20, 1 << 20, 200000, 16, (1,))
                pipe.attach_flow_control(fc)
                # the assembler's six kernels, then the ledger's five, behind the deframer (fused: nodes of the job's graph)
                assert h2dev.job_hook_counts(job) == ((before[0], before[1] + 11) if fused == "1" else before)
                with pytest.raises(g.GrdmaError):
                    pipe.attach_flow_control(fc)  # a second attach
                with pytest.raises(g.GrdmaError, match="attached to a pipe"):
                    fc.account(arena.ptr, 4, arena.ptr, 128)
            out = []
            for step in range(3):
                pipe.enqueue()
                r = pipe.sync(want_events=True)
                assert r["h2_error"] == 0
                out.append((r["event_list"], [tuple(m) for m in pipe.messages()]))
                if with_ledger:
                    rc, ev_o = orc.feed(wire, cap=len(wire) + 4096)
                    assert rc == 0
                    lens, res, exp_wire = model.call(ev_o, 0, 9, 32 * 9)
                    sl, got, got_wire = pipe.window_updates()
                    assert got == res and [n for _, n in sl] == lens and got_wire == exp_wire
            if with_ledger:
                # (the oracle parsed the wire in one piece: PAYLOAD and MSG_BYTES events follow the slices, the ledger's
                # input -- FRAME, STREAM_OPEN, STREAM_CLOSED -- does not)
                kinds = (EV_FRAME, EV_STREAM_OPEN, EV_STREAM_CLOSED)
                assert [e[:5] for e in out[0][0] if e[0] in kinds] == [e for e in ev_o if e[0] in kinds]
                st = fc.stats()
                # (the credit of steps 1 and 2 went out with step 2: step 3's bytes are still owed)
                assert st["announced"] == model.announced == (1 << 20) - res[3] and st["calls"] == 3
                fc.close()  # does nothing while attached
                assert fc.h
            runs.append(out)
            pipe.close()
            if fc:
                fc.close()
                assert fc.h is None
            job.close()
            a.close()
            parser.close()
    finally:
        if old is None:
            os.environ.pop("GRDMA_H2_PIPE_FUSED", None)
        else:
            os.environ["GRDMA_H2_PIPE_FUSED"] = old
    assert runs[0] == runs[1]


def test_chunked_deframer_path(gpu):
    warm = [frame(1, 4, 1, b"\x82")] + fast_sender_slices([100000] * 3)
    body = fast_sender_slices([100000] * 170, seed=1)
    assert len(body) >= 2048
    results = []
    for chunks in (None, False):
        h = FH(gpu, streams=(1,), stream_window=1 << 25, conn_window=1 << 26, chunks=chunks, boundary_step=True)
        h.feed(warm)
        results.append(h.feed(body))
        assert h.parser.chunk_stats() == ((1, 1) if chunks is None else (0, 0))
        h.close()
    assert results[0] == results[1] and results[0][0][3] == sum(len(s) for s in body) - 9 * (len(body) // 2)


def test_refusals_and_lifetime(gpu):
    g = gpu
    from grpc_rdma_amd import h2dev
    parser = h2dev.Parser(False)
    for kw in (dict(stream_window=0), dict(conn_window=65534), dict(conn_window=70000, conn_threshold=70001), dict(max_updates=0)):
        with pytest.raises(g.GrdmaError):
            h2dev.FlowControl(parser, **kw)
    fc = h2dev.FlowControl(parser)
    with pytest.raises(g.GrdmaError, match="a ledger already"):
        h2dev.FlowControl(parser)
    t = g.DeviceBuffer(nbytes=1024)
    with pytest.raises(g.GrdmaError, match="deframed nothing yet"):
        fc.account(t.ptr, 4, t.ptr + 256, 128)
    data, table = pack_slices([frame(0, 0, 1, b"abc")])
    buf = g.DeviceBuffer(data=data)
    parser.deframe(buf.ptr, table)
    with pytest.raises(g.GrdmaError, match="misaligned"):
        fc.account(t.ptr + 8, 4, t.ptr + 256, 128)
    with pytest.raises(g.GrdmaError, match="misaligned"):
        fc.account(t.ptr, 0, t.ptr + 256, 128)
    # the many-link calls refuse a parser that has a ledger
    other = h2dev.Parser(False)
    with pytest.raises(g.GrdmaError, match="ledger"):
        h2dev.deframe_batch([(parser, buf.ptr, table), (other, buf.ptr, table)])
    arena = g.DeviceBuffer(nbytes=1 << 16)
    a = h2dev.Assembler(parser, arena, 4 << 20, 64)
    with pytest.raises(g.GrdmaError, match="ledger"):
        h2dev.deframe_messages_batch([(parser, a, buf.ptr, table)])
    a.close()
    fc.close()
    assert fc.h is None
    fc = h2dev.FlowControl(parser)  # (the parser is free again)
    fc.close()
    # a parser closed before its ledger: the ledger refuses every call and can still be closed
    fc = h2dev.FlowControl(other)
    other.close()
    with pytest.raises(g.GrdmaError, match="parser is gone"):
        fc.account(t.ptr, 4, t.ptr + 256, 128)
    fc.close()
    assert fc.h is None
    parser.close()


def test_group_pipes_refuse_a_ledger(gpu):
    g = gpu
    from grpc_rdma_amd import h2dev, stream as gs
    parser = h2dev.Parser(False)
    assert parser.open_streams([1]) == 0
    (pipe,), (job,), keep = _pipe_setup(g, h2dev, gs, [100, 5000], 1, parser)
    pipe.close()
    fc = h2dev.FlowControl(parser)
    msgs = [(keep[0][0].ptr, 100, 1, 0)]
    with pytest.raises(g.GrdmaError, match="ledger"):
        h2dev.GroupPipe(job, [(0, msgs, parser, len(job.delivered_slices(0)), 256)])
    # a ledger of another parser than the pipe's
    p2 = h2dev.Parser(False)
    pipe = h2dev.Pipe(job, msgs, p2, len(job.delivered_slices(0)), 256)
    with pytest.raises(g.GrdmaError, match="another parser"):
        pipe.attach_flow_control(fc)
    pipe.close()
    fc.close()
    job.close()
    p2.close()
    parser.close()


def test_a_ledger_attached_elsewhere_is_refused(gpu):
    g = gpu
    from grpc_rdma_amd import h2dev, stream as gs
    parser = h2dev.Parser(False)
    assert parser.open_streams([1]) == 0
    pipes, jobs, keep = _pipe_setup(g, h2dev, gs, [100, 5000], 2, parser)
    fc = h2dev.FlowControl(parser)
    pipes[0].attach_flow_control(fc)
    with pytest.raises(g.GrdmaError, match="another pipe"):
        pipes[1].attach_flow_control(fc)
    assert fc._pipe is pipes[0]
    pipes[0].enqueue()
    assert pipes[0].sync()["h2_error"] == 0
    _, res, wire = pipes[0].window_updates()   # (the refused attach left the first one working)
    assert res[0] == 2 and res[7] == 0 and len(wire) == 26
    for p in pipes:
        p.close()
    fc.close()
    assert fc.h is None
    for j in jobs:
        j.close()
    parser.close()


def test_a_reply_pipe_refuses_a_ledger(gpu):
    g = gpu
    from grpc_rdma_amd import h2dev, stream as gs
    sizes = [3000, 0, 100]
    bodies = [bytes((j * 7 + i) % 251 for j in range(n)) for i, n in enumerate(sizes)]
    parser = h2dev.Parser(False)
    assert parser.open_streams([1]) == 0
    (pipe,), (job,), keep = _pipe_setup(g, h2dev, gs, sizes, 1, parser)
    arena = g.DeviceBuffer(nbytes=64 << 10)
    a = h2dev.Assembler(parser, arena, 4 << 20, 64)
    reply = h2dev.Reply(a, None, 16384, 64)
    pipe.attach_assembler(a)
    _, lens_back = pyorc.h2_frame_batch(bodies, [1] * len(sizes), [0] * len(sizes), 16384)
    job_back, lens_back, sent_back, keep_back = _back_job(g, gs, lens_back)
    parser_back = h2dev.Parser(False)
    assert parser_back.open_streams([1]) == 0
    rp = h2dev.Pipe.reply(job_back, reply, parser_back, len(job_back.delivered_slices(0)), 4 * len(lens_back) + 256, sent_back)
    fc = h2dev.FlowControl(parser_back)
    before = h2dev.job_hook_counts(job_back)
    with pytest.raises(g.GrdmaError, match="reply pipe"):
        rp.attach_flow_control(fc)
    assert h2dev.job_hook_counts(job_back) == before
    fc.close()
    assert fc.h is None  # (never attached: free to go)
    rp.close()
    reply.close()
    pipe.close()
    job.close()
    job_back.close()
    a.close()
    parser_back.close()
    parser.close()


def test_a_group_reply_pipe_refuses_a_ledger(gpu):
    from grpc_rdma_amd import h2dev
    E = Echo(gpu)
    fc = h2dev.FlowControl(E.parsers_back[1])
    with pytest.raises(gpu.GrdmaError, match="ledger"):
        h2dev.GroupPipe.reply(E.B.job, E.rspecs)
    assert h2dev.job_hook_counts(E.B.job) == (0, 0)
    fc.close()
    E.rp = h2dev.GroupPipe.reply(E.B.job, E.rspecs)  # (without the ledger the same specs are taken)
    E.close()
