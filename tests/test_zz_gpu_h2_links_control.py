"""Control replies on many links: the writers of a table of transports in the same four launches (k_h2_links_ctl_*,
grdma_h2_ctl_reply_batch, h2dev.control_batch).  Every item of a batch is compared exactly with its own link's
ControlModel (tests/h2_control_model.py) through reply_batch of tests/h2_control_lib.py: slices, the whole slice table and
header arena, result block, peer record and counters."""
import random

import pytest

from tests.h2_control_lib import (CH, ERR5, Target, bad_flags, bad_grpc, cut_at, data, goaway, ping, reply_batch, reply_batch_raw,
                                  settings)
from tests.h2_control_model import GOAWAY, LOST, SETTINGS_ACK, ping_ack, rst_stream
from tests.h2_device_lib import same
from tests.h2_helpers import frame

pytestmark = pytest.mark.gpu


def _flood(n):
    return b"".join(ping(0x0100000000000000 * (k % 251) + k) + data(1, bytes(k % 7)) + (settings(k % 3) if k % 97 == 5 else b"") +
                    (bad_flags(5) if k == 300 else b"") for k in range(n))


def test_nine_links_in_shuffled_order_over_two_calls(gpu):
    hs = [CH(gpu, streams=(1, 3, 5, 7), cap=640) for _ in range(9)]
    p, g = ping(0x0102030405060708), goaway(0x80000009, 0xcafe0102, bytes(range(40)))
    mixed = settings(2) + p + data(1) + bad_flags(3) + goaway(7, 2, b"bye") + ping(9, ack=True) + settings(ack=True) + settings(0)
    order_w = bad_flags(5) + ping(1) + settings(1) + bad_grpc(3, good=2, tail=30) + ping(2) + bad_flags(1) + settings(0) + bad_grpc(7, good=0)
    flood = _flood(600)
    rounds = (
        [[mixed], [mixed[i:i + 1] for i in range(len(mixed))], [settings(1) + p[:16]], [ping(4) + settings(3)[:10]],
         [goaway(1, 1) + g[:30]], [], [data(1) + data(3, b"x" * 50)], cut_at(order_w, 50, 58, 62, 80), cut_at(flood, len(flood) // 2)],
        [[ping(5, ack=True)], [], [p[16:] + ping(6)], [settings(3)[10:] + ping(7)], cut_at(g[30:] + settings(ack=True), 3),
         [], [data(3)], [bad_flags(7) + settings(1)], [settings(0) + ping(8)]])
    rng = random.Random(5)
    for n, calls in enumerate(rounds):
        for h, slices in zip(hs, calls):
            h.deframe(slices, ev_cap=16384)
        order = list(range(9))
        rng.shuffle(order)
        out = reply_batch(hs, order)
        if n == 0:
            assert out[5][1] == out[6][1] == (0, 0, 0, 0, 0, 0, 0, 0)  # no events; only DATA
            assert out[8][1][4] >= 599 and out[0][1][:6] == (4, 3, 17 + 18 + 13, 2, 1, 1)
            assert out[7][0] == (ping_ack((1).to_bytes(8, "big")) + ping_ack((2).to_bytes(8, "big")) + rst_stream(5) + SETTINGS_ACK +
                                 rst_stream(3) + rst_stream(1) + SETTINGS_ACK + rst_stream(7))
        else:
            assert out[2][0] == ping_ack(p[9:]) + ping_ack((6).to_bytes(8, "big")) and out[3][1][:6] == (2, 2, 26, 1, 1, 0)
            assert out[4][1][6] == GOAWAY and hs[4].model.peer["goaway_last_stream"] == 9 and hs[4].model.peer["goaway_call"] == 2
    for h in hs:
        h.close()


def test_batch_against_single_on_twin_parsers(gpu):
    a, b, c = (CH(gpu, streams=(1, 3, 5)) for _ in range(3))
    p = ping(0x1112131415161718)
    for slices in ([settings(1) + ping(1) + bad_flags(3) + p[:13]], [p[13:] + goaway(3, 8) + ping(2, ack=True)], [_flood(40)]):
        for h in (a, b, c):
            h.deframe(slices)
        single = a.reply()
        out = reply_batch([b, c], [1, 0])
        assert out[0] == out[1] == single
        same((b.ctl.peer(), b.ctl.stats()["calls"]), (a.ctl.peer(), a.ctl.stats()["calls"]), "twin records")
    for h in (a, b, c):
        h.close()


def test_trouble_stays_with_its_link(gpu):
    hs = [CH(gpu, streams=(1,), cap=8) for _ in range(5)]
    p = ping(0x2122232425262728)
    for h in hs:
        h.feed([settings(1) + p[:12]])
    # link 1: its event list overflows; link 2: a connection error; link 3: a cap too small; 0 and 4 are exact
    rest = [p[12:] + ping(2) + settings(0)]
    for i in (0, 2, 3, 4):
        got = hs[i].deframe(rest if i != 2 else [p[12:] + frame(6, 0, 0, b"short")])
        assert got[0] == (15 if i == 2 else 0)
    with pytest.raises(gpu.GrdmaError, match=ERR5):
        hs[1].deframe([p[12:]] + [ping(3)] * 40, ev_cap=16, checked=False)
    out = reply_batch(hs, [3, 1, 0, 2, 4], caps={3: (1, 32)}, lost=(1,))
    assert out[1][1] == (0, 0, 0, 0, 0, 0, LOST, 2) and out[2][1] == (0, 0, 0, 0, 0, 0, 0, 0)
    assert out[3][1] == (3, 2, 43, 1, 2, 0, 0, 1) and hs[3].model.carry["type"] == 6  # nothing committed
    assert out[0] == out[4] == (ping_ack(p[9:]) + ping_ack((2).to_bytes(8, "big")) + SETTINGS_ACK, (3, 2, 43, 1, 2, 0, 0, 0))
    # the overflowed item may be repeated, alone or in a batch; the others are taken
    rc, _ = reply_batch_raw(hs, [3, 0])
    assert rc == -2  # (-GRDMA_ERR_INVALID: link 0's call is taken in already; nothing ran)
    assert reply_batch(hs, [3])[3] == out[0]
    # the return value: the items without overflow
    for i in (0, 3, 4):
        hs[i].deframe([ping(1) + ping(2)])
    rc, res = reply_batch_raw(hs, [0, 3, 4], caps={3: (1, 32)})
    assert rc == 2 and [r[7] for r in res] == [0, 1, 0] and res[1][:3] == (2, 2, 34)
    for h in hs:
        h.close()


def test_256_links_and_the_refusals(gpu):
    from grpc_rdma_amd import h2dev
    hs = [CH(gpu, cap=4) for _ in range(256)]
    for i, h in enumerate(hs):
        h.deframe([ping(i) + (settings(0) if i % 3 == 0 else b"")])
    items = [(h.ctl, 0, 4, 0, 128) for h in hs]
    with pytest.raises(gpu.GrdmaError, match="BATCH_MAX"):
        h2dev.control_batch(items + items[:1])
    with pytest.raises(gpu.GrdmaError, match="BATCH_MAX"):
        h2dev.control_batch([])
    t = Target(gpu, 4)
    ok = (hs[0].ctl, t.slices.ptr, 4, t.hdr.ptr, 128)
    with pytest.raises(gpu.GrdmaError, match="twice"):
        h2dev.control_batch([ok, (hs[1].ctl, t.slices.ptr, 4, t.hdr.ptr, 128), ok])
    with pytest.raises(gpu.GrdmaError, match="without writer"):
        h2dev.control_batch([ok, (None, t.slices.ptr, 4, t.hdr.ptr, 128)])
    with pytest.raises(gpu.GrdmaError, match="null, zero or misaligned"):
        h2dev.control_batch([ok, (hs[1].ctl, t.slices.ptr + 8, 4, t.hdr.ptr, 128)])
    t.untouched("refused batches")
    order = list(range(256))
    random.Random(6).shuffle(order)
    out = reply_batch(hs, order)  # (nothing changed: every call is still to be answered)
    assert all(out[i][1][:5] == ((2, 2, 26, 1, 1) if i % 3 == 0 else (1, 1, 17, 0, 1)) for i in range(256))
    for h in hs:
        h.close()
