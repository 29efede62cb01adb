"""HTTP/2 on every link of a multi-connection job: the batched deframer (grdma_h2_deframe_batch, k_h2_deframe_links) and
the group pipe (grdma_h2_group_pipe: k_h2_frame_links -> MultiStreamJob -> k_h2_deframe_links).  The reference is the
oracle everywhere -- pyorc.H2Parser fed the bytes of the delivered slices, pyorc.h2_frame_batch for wire and slice
lengths -- and every comparison is exact.  The cases are small enough for the wave emulator (tests/test_h2_links_emu.py)."""
import random

import pytest

from tests.h2_device_lib import (ERR_CAPACITY, VEC, Links, Transport, _check_steps, _client_stream, _eight_streams, _eight_transports, cut_points,
                                 fused, oracle_events)  # noqa: F401  (fused is a fixture)
from tests.h2_helpers import PREFACE, frame, grpc_msg

pytestmark = pytest.mark.gpu


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
    ts = [Transport(gpu, "good-a", False, cut_points(_client_stream(3, [1, 3], 7), rng, 9), streams=[1, 3]),
          Transport(gpu, "too-large", False, cut_points(too_large, rng, 4), streams=[1]),
          Transport(gpu, "good-b", True, cut_points(wire8, rng, 12)),
          Transport(gpu, "bad-preface", True, cut_points(bad_preface, rng, 2)),
          Transport(gpu, "small-cap", False, cut_points(_client_stream(4, [5], 5), rng, 3), streams=[5]),
          Transport(gpu, "good-c", True, cut_points(bytes.fromhex(VEC[0]["hex"]), rng, 6))]
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
            assert got[i][1] == -ERR_CAPACITY
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


# ---- the group pipe (Links, TABLES and _check_steps: tests/h2_device_lib.py) ------------------------------------------
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
    lib = h2dev.load()
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
    lists = [cut_points(w, rng, k) for w, k in zip(wires, (6, 3, 9))]
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
