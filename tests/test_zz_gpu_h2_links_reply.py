"""Replies on many links: grdma_h2_reply_frame_batch (k_h2_reply_plan_links, k_h2_reply_emit_links over a table of
reply framers) and the group reply pipe (grdma_h2_group_pipe_create_reply).  The reference is the oracle, as in
tests/test_zz_gpu_h2_reply.py: the expected wire and slice lengths are pyorc.h2_frame_batch over the bodies the
sequential model of tests/h2_asm_model.py keeps; slice lengths, wire bytes and counters are compared exactly.  The cases
are small enough for the wave emulator (tests/test_h2_links_reply_emu.py)."""
import ctypes as C

import pytest

from tests.h2_asm_model import OK
from tests.h2_device_lib import (BATCHES, ERR_CAPACITY, SENTINEL, BackLinks, Echo, RHarness, Target, _batch, _dropped_slices, _pipe_setup,  # noqa: F401
                                 check_framed, expected_reply, fused)
from tests.h2_helpers import frame, grpc_msg

pytestmark = pytest.mark.gpu


def _assemble(hs, lists, ev_caps=None):
    """one grdma_h2_deframe_messages_batch over the harnesses; every harness's model follows (h.last = what it kept)"""
    from grpc_rdma_amd import h2dev
    items = []
    for h, slices in zip(hs, lists):
        buf, table = h.pp.upload(slices)
        h.bufs = getattr(h, "bufs", []) + [buf]
        items.append((h.parser, h.asm, buf.ptr, table))
    got = h2dev.deframe_messages_batch(items, ev_caps=ev_caps)
    for h, slices, r in zip(hs, lists, got):
        _, _, exp = h.expect(slices)
        if r[1] == -ERR_CAPACITY:  # (a call the assembler skipped: the model is not asked)
            continue
        assert [tuple(m) for m in r[1]] == [d for d, _ in exp]
    return got


# (index into BATCHES or None = the dropped-descriptor call, reply max_frame, routes or None)
EIGHT = [(1, 16384, None), (2, 16384, {1: 101}), (3, 1000, None), (4, 3, None), (5, 16384, {1: 0x01030507}),
         (6, 16384, None), (9, 5, {1: 9}), (None, 600, {1: 7})]


def _eight(gpu):
    """eight transports, assembled in one batch: [(harness, Reply, reply max_frame, routes)]"""
    from grpc_rdma_amd import h2dev
    hs, lists = [], []
    for which, _, _ in EIGHT:
        if which is None:
            hs.append(RHarness(gpu, 4096, max_msg=1200, streams=[1, 3]))
            lists.append(_dropped_slices())
        else:
            lens, max_frame = BATCHES[which]
            hs.append(RHarness(gpu, 1 << 20, max_pending=8192, streams=[1], max_frame=max_frame))
            lists.append(_batch(lens, max_frame, len(lens))[2])
    _assemble(hs, lists)
    out = []
    for h, (_, mf, routes) in zip(hs, EIGHT):
        reply = h2dev.Reply(h.asm, list(routes.items()) if routes else None, mf, 512)
        out.append((h, reply, mf, routes))
    assert {len(h.last) for h in hs} >= {1, 4, 6, 8, 9, 40}   # (different batches: the model's own counts)
    return out


def _close(cases):
    for h, reply, _, _ in cases:
        reply.close()
        h.close()


def _check_item(g, t, n, st, h, mf, routes):
    print("reply item: %d descriptors -> kept %d, %d slices, %d wire bytes" % (len(h.last), st["kept"], n, st["wire_bytes"]))
    got_lens, got_wire, _ = t.wire(n)
    check_framed(n, st, got_lens, got_wire, expected_reply(h.last, mf, routes), "reply item")
    # nothing behind what was framed, nothing behind the caps
    assert t.slices.read()[16 * n:] == bytes([SENTINEL]) * (16 * (t.cap + 4 - n))
    assert t.hdr.read()[32 * t.cap:] == bytes([SENTINEL]) * (32 * 4)


def test_batch_equals_the_oracle_per_transport(gpu):
    from grpc_rdma_amd import h2dev
    cases = _eight(gpu)
    targets = [Target(gpu, len(expected_reply(h.last, mf, routes)[1]) + 1) for h, _, mf, routes in cases]
    got = h2dev.reply_frame_batch([(reply, t.slices.ptr, t.cap, t.hdr.ptr, 32 * t.cap)
                                   for (_, reply, _, _), t in zip(cases, targets)])
    dropped = 0
    for (h, reply, mf, routes), t, (n, st) in zip(cases, targets, got):
        _check_item(gpu, t, n, st, h, mf, routes)
        assert reply.last_stats == st
        dropped += st["dropped_status"] + st["unrouted"]
    assert dropped >= 4 and len({st["frame_us"] for _, st in got}) == 1   # (the batch's time, repeated)
    _close(cases)


def test_batch_equals_the_single_call(gpu):
    from grpc_rdma_amd import h2dev
    batch, single = _eight(gpu), _eight(gpu)
    caps = [len(expected_reply(h.last, mf, routes)[1]) + 1 for h, _, mf, routes in batch]
    tb, ts = [Target(gpu, c) for c in caps], [Target(gpu, c) for c in caps]
    got = h2dev.reply_frame_batch([(reply, t.slices.ptr, t.cap, t.hdr.ptr, 32 * t.cap)
                                   for (_, reply, _, _), t in zip(batch, tb)])
    for i, ((_, reply, _, _), t) in enumerate(zip(single, ts)):
        n1, st1 = t.frame(reply)
        nb, stb = got[i]
        assert nb == n1, i
        lens_b, wire_b, _ = tb[i].wire(nb)
        lens_1, wire_1, _ = t.wire(n1)
        assert lens_b == lens_1 and wire_b == wire_1, i
        assert tb[i].hdr.read() == t.hdr.read(), i
        for k in h2dev.Reply.REPLY_STATS[:7]:
            assert stb[k] == st1[k], (i, k)
    _close(batch + single)


def test_trouble_stays_with_its_item(gpu):
    from grpc_rdma_amd import h2dev
    specs = [("good-a", [100, 0, 70000, 50], None), ("slice-cap", [3, 70000, 16379, 16380], None),
             ("max-messages", [9, 1, 0, 0, 30], None), ("skipped", [20, 21, 22, 23, 24, 25], None), ("empty", None, None),
             ("good-b", [0, 0, 0, 5, 0, 0], {1: 33})]
    hs = [RHarness(gpu, 1 << 20, streams=[1]) for _ in specs]
    lists = [_batch(lens, 16384, 7 + i)[2] if lens is not None else [] for i, (_, lens, _) in enumerate(specs)]
    res = _assemble(hs, lists, ev_caps=[None, None, None, 3, None, None])
    assert res[3][1] == -ERR_CAPACITY and res[4][1] == []
    replies = [h2dev.Reply(h.asm, list(r.items()) if r else None, 16384, 3 if name == "max-messages" else 64)
               for h, (name, _, r) in zip(hs, specs)]
    need = [len(expected_reply(h.last, 16384, r)[1]) for h, (_, _, r) in zip(hs, specs)]
    assert need[1] > 1 and len(hs[2].last) > 3
    targets = [Target(gpu, n + 1) for n in need]
    caps = [t.cap for t in targets]
    caps[1] = need[1] - 1   # one slice short
    got = h2dev.reply_frame_batch([(reply, t.slices.ptr, cap, t.hdr.ptr, 32 * t.cap)
                                   for reply, t, cap in zip(replies, targets, caps)])
    for i, (name, _, routes) in enumerate(specs):
        n, st = got[i]
        t = targets[i]
        if name.startswith("good"):
            _check_item(gpu, t, n, st, hs[i], 16384, routes)
            continue
        if name == "empty":
            assert n == 0 and st["overflow"] == 0 and st["kept"] == 0
        else:
            assert n == -ERR_CAPACITY and st["overflow"] == 1, name
            if name == "slice-cap":
                assert st["slices"] == need[1]
        assert t.slices.read() == bytes([SENTINEL]) * (16 * (t.cap + 4)), name
        assert t.hdr.read() == bytes([SENTINEL]) * (32 * (t.cap + 4)), name
    for r in replies:
        r.close()
    for h in hs:
        h.close()


# ---- the group reply pipe (Echo and BackLinks: tests/h2_device_lib.py) ------------------------------------------------
def test_group_reply_pipe(gpu, fused):
    """Four forward links and four back links, five echo steps; then link 0's parser takes a forward step of another
    shape through a second forward pipe: that spec alone reports frame overflow 2 and keeps its table; then the recorded
    shape again."""
    from grpc_rdma_amd import h2dev, stream as gs
    g = gpu
    E = Echo(g)
    E.rp = h2dev.GroupPipe.reply(E.B.job, E.rspecs)
    assert E.rp.hook_counts() == ((2, 1) if fused else (0, 0))
    E.rp.attach_assemblers(E.asms_back)
    assert E.rp.hook_counts() == ((2, 7) if fused else (0, 0))   # TWO kernels in front, 1 + 6 behind, for four links
    for k in range(5):
        tables = E.step(k)
    # a second forward pipe on link 0's parser and assembler, with messages of another shape
    other = [100, 3000, 0]
    pipes2, jobs2, keep2 = _pipe_setup(g, h2dev, gs, other, 1, E.parsers[0][0])
    pipes2[0].attach_assembler(E.las[0].asm)
    E.gp.enqueue()
    pipes2[0].enqueue()
    E.rp.enqueue()
    res = E.rp.sync()
    assert res[0]["frame_overflow"] == 2 and res[0]["h2_error"] == 0
    assert E.rp.slice_table(0) == tables[0]
    for li in (1, 2, 3):
        E.back_checked(res, li, "other")
    # (the models follow: link 0 took the group's step and then the other pipe's)
    E.forward_checked("other", overwritten=(0,))
    assert pipes2[0].sync()["h2_error"] == 0
    got = pipes2[0].messages()
    assert [(m.length, m.status) for m in got] == [(n, OK) for n in other]
    mem = keep2[-1].read()
    assert [tuple(m) for m in got] == E.advance(0, [mem[o:o + n] for o, n in jobs2[0].delivered_slices(0)])
    # link 0 re-sent its previous table: its back side received the recorded shape once more
    got0 = E.rp.messages(0)
    assert [m.length for m in got0] == [len(b) for b, _, _ in E.back[0]]
    E.seq_back[0] += len(E.back[0])
    # the recorded shape again
    E.step("again")
    E.rp.close()
    E.rp = None
    pipes2[0].close()
    for j in jobs2:
        j.close()
    E.close()


def test_refusals_and_lifetime(gpu, monkeypatch):
    from grpc_rdma_amd import h2dev
    from grpc_rdma_amd._lib import GrdmaError
    monkeypatch.delenv("GRDMA_H2_PIPE_FUSED", raising=False)
    g = gpu
    lib = h2dev.load()
    # --- the batch: nothing runs
    hs = [RHarness(g, 1 << 16, streams=[1]) for _ in range(2)]
    _assemble(hs, [[frame(0, 0, 1, grpc_msg(b"abc"))], [frame(0, 0, 1, grpc_msg(b"defg"))]])
    r0, r0b, r1 = h2dev.Reply(hs[0].asm), h2dev.Reply(hs[0].asm, [(1, 3)]), h2dev.Reply(hs[1].asm)
    t0, t1 = Target(g, 4), Target(g, 4)
    E = Echo(g)
    stats = lambda: [h.asm.stats() for h in hs] + [la.asm.stats() for la in E.las]  # noqa: E731
    before = stats()
    item = lambda r, t, **kw: (r, kw.get("sl", t.slices.ptr), kw.get("cap", t.cap), kw.get("hdr", t.hdr.ptr),  # noqa: E731
                               kw.get("hdr_cap", 32 * t.cap))

    def batch_refused(items):
        with pytest.raises(GrdmaError):
            h2dev.reply_frame_batch(items)
        assert stats() == before
        for t in (t0, t1):
            assert t.slices.read() == bytes([SENTINEL]) * (16 * (t.cap + 4))

    batch_refused([])
    assert lib.grdma_h2_reply_frame_batch(None, 1) == -2
    assert lib.grdma_h2_reply_frame_batch((h2dev.H2ReplyItem * 257)(), 257) == -2
    arr = (h2dev.H2ReplyItem * 1)()   # a NULL reply
    arr[0].d_slices_out, arr[0].slices_cap, arr[0].d_hdr_arena, arr[0].hdr_cap = t0.slices.ptr, 4, t0.hdr.ptr, 128
    assert lib.grdma_h2_reply_frame_batch(arr, 1) == -2 and b"reply" in lib.grdma_last_error()
    batch_refused([item(r0, t0), item(r1, t1), item(r0, t0)])          # a reply listed twice
    batch_refused([item(r0, t0), item(r0b, t1)])                       # two replies of one source assembler
    batch_refused([item(r0, t0), item(r1, t1, sl=0)])                  # null, zero or misaligned targets
    batch_refused([item(r0, t0), item(r1, t1, hdr=0)])
    batch_refused([item(r0, t0, cap=0), item(r1, t1)])
    batch_refused([item(r0, t0), item(r1, t1, hdr_cap=0)])
    batch_refused([item(r0, t0, sl=t0.slices.ptr + 8), item(r1, t1)])
    batch_refused([item(r0, t0), item(r1, t1, hdr=t1.hdr.ptr + 4)])
    batch_refused([item(r0, t0), item(E.replies[1], t1)])              # a source attached to a group pipe
    # --- the group reply pipe: the back job's hooks and the assemblers stay as they were
    job = E.B.job

    def refused(specs, job=job):
        with pytest.raises(GrdmaError):
            h2dev.GroupPipe.reply(job, specs)
        assert h2dev.job_hook_counts(E.B.job) == (0, 0) and E.gp.hook_counts() == (1, 7)
        assert stats() == before

    sp = E.rspecs
    refused([])
    refused(sp, job=None)
    refused([sp[0], (4,) + sp[1][1:]])                                 # a link index out of range
    refused([sp[0], (0,) + sp[1][1:]])                                 # a link listed twice
    refused([sp[0], sp[1][:2] + (None,) + sp[1][3:]])                  # no back parser
    refused([sp[0], sp[1][:2] + (sp[0][2],) + sp[1][3:]])              # a back parser listed twice
    refused([sp[0], (1, None) + sp[1][2:]])                            # a NULL reply
    refused([sp[0], (1, sp[0][1]) + sp[1][2:]])                        # a reply listed twice
    refused([sp[0], (1, r1) + sp[1][2:]])                              # a source that is not attached
    E.rp = h2dev.GroupPipe.reply(job, sp[:2])
    assert E.rp.hook_counts() == (2, 1)
    with pytest.raises(GrdmaError):                                    # a job that already carries hooks
        h2dev.GroupPipe.reply(job, sp[2:])
    B2 = BackLinks(g, E.lens[:1])
    with pytest.raises(GrdmaError):                                    # a reply bound to a pipe already
        h2dev.GroupPipe.reply(B2.job, [sp[0]])
    assert h2dev.job_hook_counts(B2.job) == (0, 0) and E.rp.hook_counts() == (2, 1) and stats() == before
    batch_refused([item(r0, t0), item(E.replies[0], t1)])              # a reply bound to a reply pipe (and an attached source)
    lib.grdma_h2_reply_destroy(E.replies[0].h)                         # (does nothing while the pipe frames through it)
    E.rp.close()
    assert h2dev.job_hook_counts(job) == (0, 0)
    # the batch still runs after the refusals
    got = h2dev.reply_frame_batch([item(r0b, t0), item(r1, t1)])
    assert [n for n, _ in got] == [2, 2] and t1.wire(2)[1] == frame(0, 0, 1, grpc_msg(b"defg"))
    assert t0.wire(2)[1] == frame(0, 0, 3, grpc_msg(b"abc"))
    # --- lifetime: the forward group pipe outlives the reply group pipe
    E.rp = h2dev.GroupPipe.reply(job, sp)
    E.rp.attach_assemblers(E.asms_back)
    E.step(0)
    E.gp.close()                                                       # does nothing while the reply group pipe exists
    assert E.gp.h is not None
    lib.grdma_h2_group_pipe_destroy(E.gp.h)
    assert E.gp.hook_counts() == (1, 7)
    E.step(1)
    E.rp.close()
    E.rp = None
    assert h2dev.job_hook_counts(job) == (0, 0)
    E.gp.enqueue()                                                     # one more forward step still works
    E.forward_checked("after")
    B2.close()
    E.close()
    for r in (r0, r0b, r1):
        r.close()
    for h in hs:
        h.close()
    assert C.sizeof(h2dev.H2ReplyItem) == 112 and C.sizeof(h2dev.H2ReplyLinkSpec) == 48
