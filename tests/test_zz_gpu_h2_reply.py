"""Replies framed on the device from received-message descriptors (grdma_h2_reply, csrc/grdma_h2_reply.h).
The reference is the oracle: the expected wire and slice lengths are pyorc.h2_frame_batch over the bodies the
sequential model of tests/h2_asm_model.py keeps (status OK, routed), on the routed stream ids, with the compressed
flags the oracle's events carry.  Slice lengths, wire bytes and counters are compared exactly."""
import ctypes as C
import os

import pytest

from oracle import pyorc
from tests.h2_asm_model import OK, TOO_LARGE, NO_SPACE, TRUNCATED
from tests.h2_device_lib import (BATCHES, ERR_CAPACITY, ERR_INVALID, SENTINEL, RHarness, Target, _back_job, _batch, _dropped_slices, _eight_streams,
                                 _pipe_setup, check_reply, device_bytes, expected_reply)
from tests.h2_helpers import frame, grpc_msg

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("reply_frame", ["same", "other"])
@pytest.mark.parametrize("lens,max_frame", BATCHES)
def test_echo_of_every_batch(gpu, lens, max_frame, reply_frame):
    from grpc_rdma_amd import h2dev
    bodies, wire, slices = _batch(lens, max_frame, len(lens))
    reply_mf = max_frame if reply_frame == "same" else (1000 if max_frame == 16384 else 16384)
    h = RHarness(gpu, 8 << 20, max_pending=8192, streams=[1], max_frame=max_frame)
    got = h.feed(slices)
    assert [m.length for m in got] == lens and all(m.status == OK for m in got)
    assert [b for _, b in h.last] == bodies
    reply = h2dev.Reply(h.asm, None, reply_mf, 8192)
    _, got_wire = check_reply(gpu, h, reply, reply_mf)
    if reply_frame == "same":  # (the echo of a batch framed by the oracle is that batch's wire)
        assert got_wire == wire
    reply.close()
    h.close()


def test_dropped_descriptors_change_the_layout(gpu):
    """OK, TOO_LARGE, TRUNCATED and NO_SPACE in one call (the constructions of test_limits and
    test_truncation_and_reuse); a TOO_LARGE message sits between an empty kept message and a non-empty kept one, so the
    inlined-slice merge crosses the dropped descriptor."""
    from grpc_rdma_amd import h2dev
    slices = _dropped_slices()
    for max_frame in (16384, 7, 600):
        h = RHarness(gpu, 4096, max_msg=1200, streams=[1, 3])
        got = h.feed(slices)
        st = [m.status for m in got]
        assert st == [OK, TOO_LARGE, OK, TRUNCATED, OK, OK, OK, NO_SPACE, NO_SPACE]
        assert [m.length for m in got][:3] == [0, 2000, 1000]  # empty kept, dropped, non-empty kept
        assert {OK, TOO_LARGE, NO_SPACE, TRUNCATED} == set(st)
        reply = h2dev.Reply(h.asm, None, max_frame, 64)
        _, _, counters = expected_reply(h.last, max_frame)
        assert counters == {"kept": 5, "dropped_status": 4, "unrouted": 0}
        check_reply(gpu, h, reply, max_frame)
        reply.close()
        h.close()


ROUTES = {1: 101, 5: 0x01030507, 9: 3, 13: 0x7FFFFFFF}


def test_routes(gpu):
    from grpc_rdma_amd import h2dev
    for seed in range(2):
        wire, parts = _eight_streams(seed)
        h = RHarness(gpu, 4 << 20, prefix=True)
        reply = h2dev.Reply(h.asm, list(ROUTES.items())[::-1], 16384, 256)
        seen = {"kept": 0, "unrouted": 0}
        for p in parts:
            h.feed([p[i:i + 1000] for i in range(0, len(p), 1000)])
            _, _, counters = expected_reply(h.last, 16384, ROUTES)
            check_reply(gpu, h, reply, 16384, ROUTES)
            for k in seen:
                seen[k] += counters[k]
        assert seen == {"kept": 16, "unrouted": 16}  # (four messages on each of eight streams, four streams routed)
        reply.close()
        h.close()


def test_route_table_errors(gpu):
    from grpc_rdma_amd import h2dev, _lib
    lib = _lib.load()
    h2dev.load()
    h = RHarness(gpu, 1 << 16, streams=[1])
    for bad in ([(1, 3), (5, 7), (1, 9)], [(0, 3)], [(1, 0)], [(2 * i + 1, 1) for i in range(4097)]):
        with pytest.raises(Exception):
            h2dev.Reply(h.asm, bad)
        arr = (h2dev.H2Route * len(bad))(*[h2dev.H2Route(a, b) for a, b in bad])
        assert not lib.grdma_h2_reply_create(h.asm.h, arr, len(bad), 16384, 64)
    assert not lib.grdma_h2_reply_create(h.asm.h, None, 2, 16384, 64)
    r = h2dev.Reply(h.asm, [(2 * i + 1, 2 * i + 3) for i in range(4096)])  # (4096 entries are accepted)
    h.feed([frame(0, 0, 1, grpc_msg(b"k" * 30))])
    check_reply(gpu, h, r, 16384, {2 * i + 1: 2 * i + 3 for i in range(4096)})
    r.close()
    h.close()


def test_cut_calls(gpu):
    """a wire cut into calls: every call's reply frames that call's descriptors only"""
    from grpc_rdma_amd import h2dev
    lens = [3, 70000, 16379, 0, 16380, 40]
    bodies, wire, _ = _batch(lens, 16384, 31)
    cuts = [5, 30, 20000, 40000, 60000, 70100, 86500, 86510, len(wire) - 20]
    bounds = [0] + cuts + [len(wire)]
    h = RHarness(gpu, 1 << 20, streams=[1])
    reply = h2dev.Reply(h.asm, None, 4096, 64)
    empty_calls, finished = 0, []
    for a, b in zip(bounds, bounds[1:]):
        h.feed([wire[a:b]])
        sl, w = check_reply(gpu, h, reply, 4096)
        finished += [body for _, body in h.last]
        if not h.last:
            empty_calls += 1
            assert sl == [] and w == b""
    assert empty_calls >= 2 and finished == bodies
    reply.close()
    h.close()


def test_caps_and_arguments(gpu):
    from grpc_rdma_amd import h2dev, _lib
    lib = _lib.load()
    h2dev.load()
    lens = [100, 0, 70000, 50]  # (no payload piece as short as an inlined slice: those are the slices of <= 23 bytes)
    bodies, wire, slices = _batch(lens, 16384, 3)
    h = RHarness(gpu, 1 << 20, streams=[1])
    h.feed(slices)
    exp_wire, exp_lens, _ = expected_reply(h.last, 16384)
    n = len(exp_lens)
    reply = h2dev.Reply(h.asm, None, 16384, 64)
    out = (C.c_uint64 * 8)()
    t = Target(gpu, n)
    # one slice short, then one header slot short: nothing behind the caps is written
    assert lib.grdma_h2_reply_frame(reply.h, t.slices.ptr, n - 1, t.hdr.ptr, 32 * n, out) == -ERR_CAPACITY
    assert int(out[6]) == 1 and int(out[3]) == n
    hdr_need = 32 * sum(1 for ln in exp_lens if ln <= 23)
    assert lib.grdma_h2_reply_frame(reply.h, t.slices.ptr, n, t.hdr.ptr, hdr_need - 1, out) == -ERR_CAPACITY
    assert t.slices.read()[16 * (n - 1):] == bytes([SENTINEL]) * (16 * 5)
    assert t.hdr.read()[hdr_need - 32:] == bytes([SENTINEL]) * (32 * (n + 4) - hdr_need + 32)
    # exactly enough
    assert lib.grdma_h2_reply_frame(reply.h, t.slices.ptr, n, t.hdr.ptr, hdr_need, out) == n
    got_lens, got_wire, _ = t.wire(n)
    assert got_lens == exp_lens and got_wire == exp_wire
    assert t.slices.read()[16 * n:] == bytes([SENTINEL]) * (16 * 4)
    assert t.hdr.read()[hdr_need:] == bytes([SENTINEL]) * (32 * (n + 4) - hdr_need)
    # more descriptors than max_messages
    small = h2dev.Reply(h.asm, None, 16384, 3)
    assert lib.grdma_h2_reply_frame(small.h, t.slices.ptr, n, t.hdr.ptr, 32 * n, out) == -ERR_CAPACITY
    small.close()
    # arguments
    f = lib.grdma_h2_reply_frame
    assert f(None, t.slices.ptr, n, t.hdr.ptr, 32 * n, out) == -ERR_INVALID
    assert f(reply.h, None, n, t.hdr.ptr, 32 * n, out) == -ERR_INVALID
    assert f(reply.h, t.slices.ptr, 0, t.hdr.ptr, 32 * n, out) == -ERR_INVALID
    assert f(reply.h, t.slices.ptr, n, None, 32 * n, out) == -ERR_INVALID
    assert f(reply.h, t.slices.ptr, n, t.hdr.ptr, 0, out) == -ERR_INVALID
    assert f(reply.h, t.slices.ptr, n, t.hdr.ptr, 32 * n, None) == -ERR_INVALID
    assert f(reply.h, t.slices.ptr + 8, n, t.hdr.ptr, 32 * n, out) == -ERR_INVALID
    assert f(reply.h, t.slices.ptr, n, t.hdr.ptr + 4, 32 * n, out) == -ERR_INVALID
    c = lib.grdma_h2_reply_create
    assert not c(None, None, 0, 16384, 64)
    assert not c(h.asm.h, None, 0, 0, 64)
    assert not c(h.asm.h, None, 0, 1 << 24, 64)
    assert not c(h.asm.h, None, 0, 16384, 0)
    assert not lib.grdma_h2_pipe_create_reply(None, 0, reply.h, h.parser.h, 1, 1, 1)
    assert lib.grdma_h2_pipe_slice_table(None, None, 0) == -ERR_INVALID
    # the assembler is not destroyed under a reply that reads it
    lib.grdma_h2_asm_destroy(h.asm.h)
    assert f(reply.h, t.slices.ptr, n, t.hdr.ptr, 32 * n, out) == n
    reply.close()
    h.close()


def test_end_to_end_standalone(gpu):
    """receive -> assemble -> frame the reply -> through a connected pair -> a second parser and assembler: the
    messages there are the original bodies; the first assembler is released only after that"""
    g = gpu
    from grpc_rdma_amd import h2dev
    lens = [1 << 20, 70000, 0, 5, 300000, 0, 0, 17]
    bodies, wire, slices = _batch(lens, 16384, 21)
    h1 = RHarness(g, 4 << 20, streams=[1])
    h1.feed(slices)
    reply = h2dev.Reply(h1.asm, [(1, 7)], 16384, 64)
    sl, echoed = check_reply(g, h1, reply, 16384, {1: 7})
    a, b = g.Pair(4 << 20, 4095), g.Pair(4 << 20, 4095)
    g.connect_pairs(a, b)
    delivered = []
    steps, done = a.endpoint_write(sl)
    while True:
        got, wb = b.endpoint_read(8192)
        delivered += got
        if done and not got:
            break
        if not done:
            steps, done = a.endpoint_write_continue()
    assert b"".join(delivered) == echoed
    h2 = RHarness(g, 4 << 20, streams=[7])
    back = h2.feed(delivered)
    assert [(m.stream_id, m.status) for m in back] == [(7, OK)] * len(lens)
    assert [h2.asm.view(m) for m in back] == bodies and [x for _, x in h2.last] == bodies
    h1.release()
    assert h1.asm.stats()["bytes_in_use"] == 0
    reply.close()
    h1.close()
    h2.close()


@pytest.mark.parametrize("fused", ["1", "0"])
def test_reply_pipe(gpu, fused):
    g = gpu
    from grpc_rdma_amd import h2dev, stream as gs, _lib
    lib = _lib.load()
    sizes = [70000, 1, 16379, 0, 200000, 5000]
    other = [100, 3000, 0]
    bodies = [bytes((j * 7 + i) % 251 for j in range(n)) for i, n in enumerate(sizes)]
    old = os.environ.get("GRDMA_H2_PIPE_FUSED")
    os.environ["GRDMA_H2_PIPE_FUSED"] = fused
    try:
        parser = h2dev.Parser(False)
        assert parser.open_streams([1]) == 0
        pipes, jobs, keep = _pipe_setup(g, h2dev, gs, sizes, 2, parser)
        pipes2, jobs2, keep2 = _pipe_setup(g, h2dev, gs, other, 1, parser)
        arena = g.DeviceBuffer(nbytes=512 << 10)
        a = h2dev.Assembler(parser, arena, 4 << 20, 4096)
        reply = h2dev.Reply(a, None, 16384, 64)
        for p in pipes + pipes2:
            p.attach_assembler(a)
        # (the reply's slice list, merges behind the empty message included: the oracle's framing of the step)
        exp_wire, lens_back = pyorc.h2_frame_batch(bodies, [1] * len(sizes), [0] * len(sizes), 16384)
        job_back, lens_back, sent_back, keep_back = _back_job(g, gs, lens_back)
        parser_back = h2dev.Parser(False)
        assert parser_back.open_streams([1]) == 0
        rp = h2dev.Pipe.reply(job_back, reply, parser_back, len(job_back.delivered_slices(0)), 4 * len(lens_back) + 256,
                              sent_back)
    finally:
        if old is None:
            os.environ.pop("GRDMA_H2_PIPE_FUSED", None)
        else:
            os.environ["GRDMA_H2_PIPE_FUSED"] = old
    arena_back = g.DeviceBuffer(nbytes=512 << 10)
    a_back = h2dev.Assembler(parser_back, arena_back, 4 << 20, 4096)
    rp.attach_assembler(a_back)
    exp_lens = lens_back
    step_bytes = sum(((n + 255) // 256) * 256 for n in sizes)

    def step(fwd, k):
        fwd.enqueue()
        rp.enqueue()
        r = rp.sync()
        assert r["h2_error"] == 0 and r["frame_overflow"] == 0 and r["framed"] == len(lens_back)
        got = rp.messages()
        assert [(m.status, m.length, m.stream_id) for m in got] == [(OK, n, 1) for n in sizes]
        assert [m.seq for m in got] == list(range(k * len(sizes), (k + 1) * len(sizes)))
        assert [a_back.view(m) for m in got] == bodies
        fr = fwd.sync()
        assert fr["h2_error"] == 0
        assert [a.view(m) for m in fwd.messages()] == bodies
        assert a.stats()["bytes_in_use"] <= step_bytes + max(sizes)

    for k in range(5):
        step(pipes[k % 2], k)
    # the slice table the back job sends from is the oracle's framing of the forward step's messages
    table = rp.slice_table()
    assert [ln for _, ln in table] == exp_lens
    assert b"".join(device_bytes(g, p, ln) for p, ln in table) == exp_wire
    # a forward step of another shape: nothing is written, the job re-sends its previous table, overflow 2
    pipes2[0].enqueue()
    rp.enqueue()
    r = rp.sync()
    assert r["frame_overflow"] == 2 and r["h2_error"] == 0
    assert rp.slice_table() == table
    assert [m.length for m in pipes2[0].messages()] == other
    # the recorded shape again
    step(pipes[1], 6)
    # a standalone call on a reply whose source assembles in pipes is refused
    t = Target(g, len(lens_back) + 1)
    with pytest.raises(Exception):
        t.frame(reply)
    # the forward pipes outlive the reply pipe: their destroy does nothing while it exists
    with pytest.raises(Exception):
        pipes[0].close()
    lib.grdma_h2_pipe_destroy(pipes[0].h)
    lib.grdma_h2_reply_destroy(reply.h)
    step(pipes[0], 7)
    rp.close()
    reply.close()
    for p in pipes + pipes2:
        p.close()
    for j in jobs + jobs2 + [job_back]:
        j.close()
    a.close()
    a_back.close()
    parser.close()
    parser_back.close()
