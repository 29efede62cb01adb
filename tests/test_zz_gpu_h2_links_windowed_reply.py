"""Replies under the peer's windows on many links: grdma_h2_reply_frame_windowed_batch (k_h2_links_wr_queue,
k_h2_links_sw_plan, k_h2_links_sw_emit, k_h2_links_wr_commit: four launches however many links).  Every item of a batch
is compared exactly with its own link's model, as a single call is (frame_batch of tests/h2_windowed_reply_lib.py), and
with a twin that is framed by single calls."""
import random

import pytest

from tests.h2_device_lib import ERR_CAPACITY, same
from tests.h2_send_lib import body, window_update
from tests.h2_windowed_reply_lib import WH, data, frame_batch

pytestmark = pytest.mark.gpu


def _round(rng, k):
    """the messages one link receives in a round"""
    return [f for i in range(rng.randrange(0, 6)) for f in
            data(rng.choice((1, 3, 5)), body(rng.choice((0, 1, 4, 30, 200, 700)), 10 * k + i), rng.randrange(2))]


def _credit(rng):
    return [b"".join(window_update(s, rng.choice((1, 5, 40, 300))) for s in (0, 1, 3, 5) if rng.randrange(3))]


def test_nine_links_three_rounds_against_single_calls(gpu):
    rng = random.Random(5)
    windows = [(rng.choice((0, 3, 6, 40, 65535)), rng.choice((7, 100, 65535))) for _ in range(9)]
    frames = [rng.choice((5, 6, 23, 16384)) for _ in range(9)]

    def links():
        return [WH(gpu, initial_window=w, conn_window=c, max_frame=mf) for (w, c), mf in zip(windows, frames)]
    batch, single = links(), links()
    for rnd in range(3):
        order = list(range(9))
        rng.shuffle(order)
        recv = [_round(rng, 9 * rnd + li) for li in range(9)]
        cred = [_credit(rng) for li in range(9)]
        for hs in (batch, single):
            for li in order:
                if recv[li] or rnd == 0:
                    hs[li].receive(recv[li])
                if cred[li][0]:
                    hs[li].credit(cred[li])
        got = frame_batch([batch[li] for li in order])
        for li, (wire, res) in zip(order, got):
            same((wire, res), single[li].frame(), "round %d, link %d: the batch against the single call" % (rnd, li))
            same(batch[li].reply.pending(), single[li].reply.pending(), "round %d, link %d: the queues" % (rnd, li))
        assert any(res[1] for _, res in got) and any(res[0] for _, res in got)
    for h in batch + single:
        h.close()


def test_source_calls_of_a_batch_are_counted(gpu):
    # proxies whose sources are assembled by grdma_h2_deframe_messages_batch: each of its calls is taken once
    from grpc_rdma_amd import h2dev
    hs = [WH(gpu, streams=(1, 3), routes={1: 11, 3: 13}, out_streams=(11, 13), initial_window=50 * (li + 1)) for li in range(3)]
    for rnd in range(2):
        lists = [data(1, body(120, li + rnd)) + data(3, body(40, li)) for li in range(3)]
        items, bufs = [], []
        for h, slices in zip(hs, lists):
            buf, table = h.r.pp.upload(slices)
            bufs.append(buf)
            items.append((h.r.parser, h.r.asm, buf.ptr, table))
        got = h2dev.deframe_messages_batch(items)
        for h, slices, r in zip(hs, lists, got):
            _, _, exp = h.r.expect(slices)
            same([tuple(m) for m in r[1]], [d for d, _ in exp], "descriptors")
            h.model.source_call(h.r.last)
        res = frame_batch(hs)
        assert [r[8] for _, r in res] == [2, 2, 2] and all(r[13] == 0 for _, r in res)
    for h in hs:
        h.close()


def test_trouble_stays_with_its_link(gpu):
    names = ["good-a", "slice-cap", "queue-full", "lost", "good-b"]
    hs = [WH(gpu, initial_window=10, conn_window=65535, max_frame=16, max_pending=2 if n == "queue-full" else 64) for n in names]
    for h in hs:
        h.receive(data(1, body(30, 1)) + data(3, body(30, 2)))
    hs[3].receive(data(5, body(9, 3)))  # (lost: two source calls, none taken)
    first = frame_batch(hs)
    assert [r[7] for _, r in first] == [0] * 5 and [r[13] for _, r in first] == [0, 0, 0, 1, 0]
    for h in hs:
        h.credit([window_update(1, 100) + window_update(3, 100)])
    hs[2].receive(data(5, body(30, 4)))  # (two wait, one arrives: one more than max_pending)
    hs[1].receive(data(5, body(100, 5)))
    kw = [{}, {"cap": 3}, {}, {}, {"pending_only": True}]
    got = frame_batch(hs, kw)
    assert [r[7] for _, r in got] == [0, 1, 2, 0, 0] and got[2][1][1] == 3
    # (the lost link took its second call only: stream 5's message, which got no credit)
    assert [r[:2] for _, r in got] == [(2, 0), (0, 2), (0, 3), (0, 1), (2, 0)] and got[3][1][13] == 1
    # the repeats: with room, and the queue alone
    got = frame_batch(hs[1:3], [{}, {"pending_only": True}])
    assert [r[7] for _, r in got] == [0, 0] and got[0][1][8] == 1 and got[1][1][:2] == (2, 0)
    for h in hs:
        h.close()


def test_256_links(gpu):
    hs = [WH(gpu, streams=(1,), arena_bytes=1024, initial_window=5 + li % 7, conn_window=65535, cap=8) for li in range(256)]
    for li, h in enumerate(hs):
        h.receive(data(1, body(1 + li % 5, li)))
    got = frame_batch(hs)
    assert [r[5] for _, r in got] == [min(5 + li % 7, 6 + li % 5) for li in range(256)]
    for h in hs:
        h.credit([window_update(1, 20)])
    got = frame_batch(hs, [{"pending_only": True}] * 256)
    assert all(r[1] == 0 and r[12] == 1 for _, r in got)
    for h in hs:
        h.close()


def test_refusals(gpu):
    g = gpu
    from grpc_rdma_amd import h2dev
    lib = h2dev.load()
    assert lib.grdma_h2_reply_frame_windowed_batch(None, 1) == -2
    assert lib.grdma_h2_reply_frame_windowed_batch((h2dev.H2WrItem * 257)(), 257) == -2
    a, b = WH(g), WH(g)
    for h in (a, b):
        h.receive(data(1, body(10, 1)))
    t = g.DeviceBuffer(nbytes=16384)
    ok = lambda h, k: (h.reply, t.ptr + 4096 * k, 8, t.ptr + 4096 * k + 2048, 128, False)  # noqa: E731
    for items, why in (([(None,) + ok(a, 0)[1:]], "no reply"),
                       ([ok(a, 0), ok(a, 1)], "same reply twice"),
                       ([ok(a, 0), (b.reply, t.ptr + 8, 8, t.ptr + 2048, 128, False)], "misaligned"),
                       ([ok(a, 0), (b.reply, t.ptr + 4096, 0, t.ptr + 6144, 128, False)], "misaligned")):
        with pytest.raises(g.GrdmaError):
            h2dev.reply_frame_windowed_batch(items)
        assert why.encode() in lib.grdma_last_error()
    plain = h2dev.Reply(a.r.asm, None, 16384)  # (a second reply of a's source, attached to windows of its own: refused)
    with pytest.raises(g.GrdmaError):
        h2dev.reply_frame_windowed_batch([ok(a, 0), (plain,) + ok(b, 1)[1:]])
    assert b"no send windows attached" in lib.grdma_last_error()
    plain.close()
    # nothing ran: both links answer as if no batch had been tried
    got = frame_batch([a, b])
    assert [r[:2] for _, r in got] == [(1, 0), (1, 0)]
    with pytest.raises(g.GrdmaError):  # (an overflowing item is -GRDMA_ERR_CAPACITY in its own n_slices, not an error)
        h2dev.reply_frame_windowed_batch([])
    a.receive(data(1, body(100, 2)))
    res = h2dev.reply_frame_windowed_batch([(a.reply, t.ptr, 1, t.ptr + 2048, 32, False)])
    assert res[0][0] == -ERR_CAPACITY and res[0][1]["overflow"] == 1
    a.close()
    b.close()
