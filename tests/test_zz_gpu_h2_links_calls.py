"""The call tables of many links stepped in one call, eight launches however many (k_h2_links_calls_*,
grdma_h2_calls_step_batch, h2dev.calls_step_batch).  Every item of a batch is compared exactly with its own table's
CallsModel (tests/h2_calls_model.py), stepped independently in item order, through step_batch of
tests/h2_links_calls_lib.py: the dispatch table, the segment words and the done list whole -- what is not written keeps
its fill -- the result block, the dump and the counters; what a test asserts beside that is what the case is about.  The
shapes are the edges of a link's share of the grid: four workgroups on the device (a run is ceil(n / 4) rounded up to 256,
the run loop's second pass first happens at 1025), two under the emulator (at 513); the link under test stands between
two small ones, so a neighbour's workgroups would show in its targets."""
import random

import pytest

from tests.h2_calls_lib import cluster_id
from tests.h2_calls_model import (BAD_INPUT, COMPRESSED, DEADLINE, ERR_METHOD, ERR_STREAM, FIRST, LAST, LEFT, LOST, NO_CALL, READS_CLOSED,
                                  closed, message, request)
from tests.h2_hpenc_lib import ERR2
from tests.h2_links_calls_lib import CH, Link, Out, Tables, compare, prepare, step_batch, unchanged

pytestmark = pytest.mark.gpu

INVALID = -2
COUNTS = [0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049]


def sid(k):
    return 2 * k + 1


def reason(rec):
    return rec[6] >> 8 & 0xff


def small(k, now=0):
    """a small link's step: two opens, three messages (one an orphan), a close"""
    a, b = sid(100 * k + 1), sid(100 * k + 2)
    return dict(reqs=[request(a, 1), request(b, 2)], msgs=[message(a, length=k + 1), message(sid(9999)), message(b, length=7)],
                events=[closed(a, False)], now=now)


def between(gpu, table_slots=16, nmethods=3):
    """three tables: the one under test between two small ones"""
    return [CH(gpu, 16, 3), CH(gpu, table_slots, nmethods), CH(gpu, 16, 3)]


def close(hs):
    for h in hs:
        h.close()


# ---- counts -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", COUNTS)
def test_record_message_and_event_counts_in_the_middle_link(gpu, n):
    hs = between(gpu, table_slots=4096)
    # n records: every third no request, every fifth refused
    reqs = [request(sid(k), k % 3, kind=2 if k % 3 == 2 else 1, verdict=6 if k % 5 == 4 else 0) for k in range(n)]
    opened = sum(1 for k in range(n) if k % 3 != 2 and k % 5 != 4)
    count, out, _ = step_batch(hs, [0, 1, 2], steps={0: small(1), 1: dict(reqs=reqs, msgs=[message(sid(k)) for k in range(0, n, 7)]), 2: small(2)})
    assert count == 3 and out[1][3][0] == opened and out[1][3][5] == opened and out[0][3][:3] == out[2][3][:3] == (2, 2, 1)
    # n messages: ten streams and an unknown one, interleaved
    msgs = [message(sid(i * 7 % 11), length=i, offset=256 * i, compressed=i % 4 == 1) for i in range(n)]
    count, out, _ = step_batch(hs, [0, 1, 2], steps={0: small(3), 1: dict(msgs=msgs), 2: small(4)})
    assert count == 3 and out[1][3][1] + out[1][3][2] == n and out[1][1][-1] == n
    # n events: reads closed then left, other kinds and streams without entry between
    events = [closed(sid(j // 2), j % 2) if j % 3 else (5, 0, 0, sid(j // 2), 0, 0) for j in range(n)]
    count, out, _ = step_batch(hs, [0, 1, 2], steps={0: small(5), 1: dict(events=events), 2: small(6)})
    disp, segs, done, res = out[1]
    assert count == 3 and res[3] == len(done) and res[5] == opened - sum(1 for d in done if d[5] & 0xff == LEFT)
    close(hs)


# ---- sequences within a call ----------------------------------------------------------------------------------------------------
def test_one_stream_in_every_run_of_its_link_over_two_steps(gpu):
    hs = between(gpu, nmethods=2)
    step_batch(hs, [0, 1, 2], steps={0: small(1), 1: dict(reqs=[request(1, 1), request(3, 0), request(5, 0)]), 2: small(2)})
    # 1000 messages: four runs of 256 on the device, two of 512 under the emulator; stream 1 at both ends of every one
    at = (0, 255, 256, 300, 511, 512, 767, 768, 999)
    msgs = [message(1 if i in at else 3 + 2 * (i % 2), length=i) for i in range(1000)]
    count, out, _ = step_batch(hs, [0, 1, 2], steps={0: small(3), 1: dict(msgs=msgs), 2: small(4)})
    mine = [r for r in out[1][0] if r[3] == 1]
    assert [r[4] for r in mine] == list(at) and [r[7] for r in mine] == list(range(9))
    assert [r[6] & FIRST for r in mine] == [FIRST] + [0] * 8 and not any(r[6] & LAST for r in out[1][0])
    # the next batch continues the count; the close comes with it: LAST on the last one, FIRST nowhere on the stream
    count, out, _ = step_batch(hs, [0, 1, 2], steps={1: dict(msgs=msgs, events=[closed(1, False)])})
    mine = [r for r in out[1][0] if r[3] == 1]
    assert [(r[4], r[7]) for r in mine] == list(zip(at, range(9, 18))) and [r[6] & (FIRST | LAST) for r in mine] == [0] * 8 + [LAST]
    assert not any(r[6] & LAST for r in out[1][0] if r[3] != 1) and out[1][2] == [(0, 2 * sum(at), 1, 1, 18, READS_CLOSED)]
    close(hs)


# ---- duplicates ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("a,b", [(255, 256), (511, 512), (0, 999)])
def test_a_request_twice_across_a_runs_edge_and_across_steps(gpu, a, b):
    hs = between(gpu, table_slots=2048, nmethods=2)
    reqs = [request(sid(k + 10)) for k in range(1000)]
    reqs[a], reqs[b] = request(5, 1, encoding=1), request(5, 0)  # the first wins: method 1, gzip
    count, out, _ = step_batch(hs, [0, 1, 2], steps={0: small(1), 1: dict(reqs=reqs, msgs=[message(5, compressed=True)]), 2: small(2)})
    disp, segs, done, res = out[1]
    assert res[0] == 999 and disp[0][5] == 1 and disp[0][6] == FIRST | COMPRESSED | 1 << 16 and disp[0][2] == a
    # ... and across steps: the entry stays what it was
    count, out, _ = step_batch(hs, [1], steps={1: dict(reqs=[request(5, 0)], msgs=[message(5)])})
    disp, segs, done, res = out[1]
    assert count == 1 and res[0] == 0 and (disp[0][5], disp[0][7]) == (1, 1)
    close(hs)


# ---- methods ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nmethods", [0, 1, 4096])
def test_methods(gpu, nmethods):
    hs = between(gpu, nmethods=nmethods)
    methods = [nmethods - 1, 0, nmethods // 2] if nmethods else []
    reqs = [request(sid(k), m) for k, m in enumerate(methods)]
    msgs = [message(sid(i % 4), length=i) for i in range(300)]  # (sid(3) has no call)
    count, out, _ = step_batch(hs, [0, 1, 2], steps={0: small(1), 1: dict(reqs=reqs, msgs=msgs), 2: small(2)})
    disp, segs, done, res = out[1]
    assert count == 3 and len(segs) == nmethods + 2 and segs[-1] == 300 and res[2] == (75 if nmethods else 300)
    if nmethods == 4096:
        assert (segs[1], segs[2048], segs[2049], segs[4095], segs[4096]) == (75, 75, 150, 150, 225)
    close(hs)


def test_everything_orphaned(gpu):
    hs = between(gpu, nmethods=2)
    count, out, _ = step_batch(hs, [0, 1, 2], steps={0: small(1), 1: dict(msgs=[message(sid(i % 5), status=i % 4) for i in range(300)]), 2: small(2)})
    assert count == 3 and out[1][1] == [0, 0, 0, 300] and out[1][3][1:3] == (0, 300)
    close(hs)


# ---- the table ----------------------------------------------------------------------------------------------------------------
CLUSTER = [cluster_id(hm, k) for hm in (14, 15, 0, 1) for k in range(2)]  # eight ids, two on each of the homes 14, 15, 0, 1


def test_half_the_slots_and_one_more_lost_sticks_for_that_table_alone(gpu):
    hs = between(gpu)
    nine = [request(sid(k), k % 3) for k in range(9)]
    count, out, _ = step_batch(hs, [0, 1, 2], steps={0: small(1), 1: dict(reqs=nine, msgs=[message(sid(8)), message(sid(7))]), 2: small(2)})
    assert count == 3 and out[1][3][0] == 8 and out[1][3][6] == LOST and out[0][3][6] == out[2][3][6] == 0 and reason(out[1][0][-1]) == NO_CALL
    # sticky, for that table; a single step sees it too
    count, out, _ = step_batch(hs, [2, 1, 0], steps={0: small(3), 1: dict(events=[closed(sid(0), True)]), 2: small(4)})
    assert out[1][3][5:7] == (7, LOST) and out[0][3][6] == out[2][3][6] == 0
    disp, segs, done, res = hs[1].step([request(sid(8))], [message(sid(8))])
    assert res[0] == 1 and res[6] == LOST and hs[0].dev.stats()["lost"] == 0
    close(hs)


def test_opens_and_lefts_clustered_on_the_wrap(gpu):
    hs = between(gpu, nmethods=2)
    count, out, _ = step_batch(hs, [0, 1, 2], steps={0: small(1), 1: dict(reqs=[request(s, i % 2) for i, s in enumerate(CLUSTER)],
                                                                              msgs=[message(s, length=s) for s in CLUSTER]), 2: small(2)})
    assert out[1][3][:2] == (8, 8) and not out[1][3][6]
    # two leave; in the batch behind, two others come on the same homes and everyone gets a message
    step_batch(hs, [0, 1, 2], steps={1: dict(events=[closed(CLUSTER[0], True), closed(CLUSTER[3], True)])})
    new = [cluster_id(14, 2), cluster_id(15, 2)]
    count, out, _ = step_batch(hs, [0, 1, 2], steps={0: small(3), 1: dict(reqs=[request(s) for s in new], msgs=[message(s) for s in new + CLUSTER]), 2: small(4)})
    disp, segs, done, res = out[1]
    assert res[0] == 2 and res[5] == 8 and sorted(r[3] for r in disp if reason(r) == NO_CALL) == sorted([CLUSTER[0], CLUSTER[3]])
    close(hs)


# ---- single and batch steps on one table -------------------------------------------------------------------------------------
def traffic(t):
    """a step of mixed traffic: opens (one twice, some with a deadline), messages to this step's and the last step's
    calls, closes of the last step's calls"""
    base = 20 * t
    reqs = [request(sid(base + k), k % 3, timeout=30 if k % 4 == 0 else None, encoding=k % 2) for k in range(12)] + [request(sid(base + 3), 1)]
    msgs = [message(sid(abs(base + i * 5 % 14 - 4)), length=i + t, compressed=i % 3 == 0, status=1 if i % 17 == 16 else 0) for i in range(300)]
    events = [closed(sid(max(0, base + k - 20)), k % 2 == 0) for k in range(12)] + [closed(sid(base + 1), False)]
    return dict(reqs=reqs, msgs=msgs, events=events, now=25 * t)


def test_twin_tables_single_and_batch_steps_alternating(gpu):
    a, b, other = CH(gpu, 256, 3), CH(gpu, 256, 3), CH(gpu, 16, 3)
    for t in range(10):  # five steps, then five with the roles swapped on the same two tables
        single, batched = (a, b) if t < 5 else (b, a)
        one = single.step(**traffic(t))
        count, out, _ = step_batch([other, batched], [0, 1], steps={0: small(t % 3, now=t), 1: traffic(t)})
        assert count == 2 and out[1] == one, t
        da, db = a.dev.dump(), b.dev.dump()
        assert da[0].tobytes() == db[0].tobytes() and da[1] == db[1], t
        sa, sb = a.dev.stats(), b.dev.stats()
        assert {k: v for k, v in sa.items() if k != "kernel_us"} == {k: v for k, v in sb.items() if k != "kernel_us"}, t
    close([a, b, other])


def test_nine_links_in_shuffled_order_over_three_batches(gpu):
    hs = [CH(gpu, 16, 3) for _ in range(9)]
    rng = random.Random(9)
    for t in range(3):
        order = list(range(9))
        rng.shuffle(order)
        steps = {i: small(10 * t + i, now=i) for i in order if (i + t) % 4}  # (the others: an empty step)
        for i in steps if t else ():
            steps[i]["events"].append(closed(sid(100 * (10 * (t - 1) + i) + 2), True))  # (the last batch's second call leaves)
        count, out, _ = step_batch(hs, order, steps=steps)
        assert count == 9 and all(out[i][3][0] == (2 if i in steps else 0) for i in order), t
    close(hs)


# ---- trouble stays with its item -------------------------------------------------------------------------------------------------
def test_trouble_stays_with_its_item_and_the_repeat_is_exact(gpu):
    hs = [CH(gpu, 16, 2) for _ in range(6)]
    step_batch(hs, range(6), steps={i: dict(reqs=[request(sid(k), k % 2) for k in range(3)]) for i in range(6)})
    msgs = [message(sid(k % 4), length=k) for k in range(5)]
    good = dict(reqs=[request(sid(10), 1)], msgs=msgs, events=[closed(sid(1), False)])
    late = dict(reqs=[request(sid(11), timeout=0)], msgs=msgs, events=[closed(sid(0), True), closed(sid(1), False)], now=5)
    steps = {0: dict(reqs=[request(sid(10)), request(0)], msgs=msgs),        # a bad stream
             1: good,
             2: dict(reqs=[request(sid(10), 2), request(0, 9)], msgs=msgs),  # a bad method, in front of a bad stream
             3: good,                                                        # with a dispatch cap too small
             4: good,
             5: late}                                                        # with a done cap too small
    count, out, links = step_batch(hs, range(6), steps=steps, caps={3: (4, None), 5: (None, 2)})
    assert count == 2 and out[1] == out[4] and out[1][3][:4] == (1, 4, 1, 1)
    assert out[0][3] == (0, 0, 0, 0, 0, 0, BAD_INPUT | ERR_STREAM << 8 | 1 << 32, 0) and out[2][3] == (0, 0, 0, 0, 0, 0, BAD_INPUT | ERR_METHOD << 8, 0)
    assert out[3][3] == out[1][3][:7] + (1,) and out[5][3] == (1, 4, 1, 3, 1, 3, 0, 1)
    assert [hs[i].dev.stats()["steps"] for i in range(6)] == [1, 2, 1, 1, 2, 1]
    # repeated with good input or larger caps, in a later batch and alone: what a never-refused step gives
    count, again, _ = step_batch(hs, [5, 0, 2], steps={0: good, 2: good, 5: late})
    assert count == 3 and again[0] == again[2] == out[1] and again[5][3] == (1, 4, 1, 3, 1, 3, 0, 0)
    count, again, _ = step_batch(hs, [3], steps={3: good})
    assert count == 1 and again[3] == out[1]
    close(hs)


def test_a_batch_in_which_no_item_commits_moves_no_counter(gpu):
    hs = [CH(gpu, 16, 3) for _ in range(3)]
    count, _, _ = step_batch(hs, range(3), steps={i: small(1) for i in range(3)})
    before = [h.dev.stats() for h in hs]
    assert count == 3 and [s["steps"] for s in before] == [1, 1, 1]
    count, out, _ = step_batch(hs, range(3), steps={0: dict(reqs=[request(0)]), 1: dict(msgs=[message(1)] * 3), 2: dict(reqs=[request(9, 3)])},
                               caps={1: (2, None)})
    after = [h.dev.stats() for h in hs]
    assert count == 0 and [{k: v for k, v in s.items() if k != "kernel_us"} for s in after] == [{k: v for k, v in s.items() if k != "kernel_us"} for s in before]
    close(hs)


def test_an_empty_item_is_a_step_and_expires_against_its_own_clock(gpu):
    from grpc_rdma_amd import h2dev
    hs = [CH(gpu, 16, 3) for _ in range(2)]
    step_batch(hs, [0, 1], steps={0: dict(reqs=[request(1, timeout=100)]), 1: small(0)})
    count, out, _ = step_batch(hs, [0, 1], steps={0: dict(now=100)})
    assert count == 2 and out[0][2] == [(0, 0, 1, 0, 0, DEADLINE)] and out[0][3] == (0, 0, 0, 1, 1, 1, 0, 0) and out[1][3] == (0, 0, 0, 0, 0, 2, 0, 0)
    assert [h.dev.stats()["steps"] for h in hs] == [2, 2]
    # ... with no input tables at all, and alone
    o = Out(gpu, 1, 1, 3)
    count, got = h2dev.calls_step_batch([(hs[1].dev, 0, 0, 0, 0, 0, 0, 0, 7) + o.args()])
    hs[1].model.step([], [], [], [], 7, 1, 1)
    assert (count, got) == (1, [(0, 0, 0, 0, 0, 2, 0, 0)]) and hs[1].dev.stats()["steps"] == 3
    assert o.segments.read() == bytes(20) + bytes([0xA5]) * 16 and o.dispatch.read() == bytes([0xA5]) * (48 * 3) and o.done.read() == bytes([0xA5]) * (32 * 3)
    hs[1].check()
    close(hs)


def test_per_item_clocks(gpu):
    hs = [CH(gpu, 16, 1) for _ in range(4)]
    step_batch(hs, range(4), steps={i: dict(reqs=[request(1, timeout=100), request(3, timeout=120)], now=10 * i) for i in range(4)})
    # deadlines at 100 + 10 i and 120 + 10 i; the clocks: 99, 110, 119, 150
    clocks = (99, 110, 119, 150)
    count, out, _ = step_batch(hs, [3, 1, 0, 2], steps={i: dict(msgs=[message(1), message(3)], now=clocks[i]) for i in range(4)})
    assert count == 4 and [out[i][3][4] for i in range(4)] == [0, 1, 0, 2] and [out[i][3][1] for i in range(4)] == [2, 1, 2, 0]
    close(hs)


# ---- many items ----------------------------------------------------------------------------------------------------------------
def test_one_set_of_input_tables_shared_by_sixteen_items(gpu):
    hs = [CH(gpu, 16, 3) for _ in range(16)]
    s = dict(reqs=[request(sid(k), k % 3, timeout=5 * k) for k in range(6)], msgs=[message(sid(i % 7), length=i) for i in range(70)],
             events=[closed(sid(2), False), closed(sid(4), True)])
    t = Tables(gpu, [r[0] for r in s["reqs"]], [r[1] for r in s["reqs"]], s["msgs"], s["events"])
    count, out, links = step_batch(hs, range(16), steps={i: dict(s, now=i) for i in range(16)}, device={i: t.args() for i in range(16)})
    assert count == 16 and all(links[i].inp is None for i in range(16))
    # (the same records everywhere; the deadlines in the dumps, which step_batch compared, move with the item's clock)
    assert all(out[i] == out[0] for i in range(16)) and out[0][3] == (6, 50, 20, 3, 1, 5, 0, 0)
    assert [int(h.dev.dump()[0]["deadline_ns"][1]) for h in hs] == [i + 5 for i in range(16)]
    close(hs)


@pytest.mark.parametrize("n", [33, 256])
def test_many_items(gpu, n):
    hs = [CH(gpu, 16, 3) for _ in range(n)]
    count, out, _ = step_batch(hs, range(n), steps={i: small(i % 50, now=i) for i in range(n) if i % 5})
    assert count == n and all(out[i][3][:3] == ((2, 2, 1) if i % 5 else (0, 0, 0)) for i in range(n))
    order = list(range(n - 1, -1, -1))
    count, out, _ = step_batch(hs, order, steps={i: dict(msgs=[message(sid(100 * (i % 50) + 1), length=i)]) for i in range(n)})
    assert count == n and all(out[i][3][1] == (1 if i % 5 else 0) for i in range(n))
    close(hs)


# ---- the chain on device tables ---------------------------------------------------------------------------------------------------
def test_deframe_decode_batch_read_batch_and_route_on_three_links(gpu):
    import struct
    from grpc_rdma_amd import h2dev
    from tests.h2_device_lib import device_bytes
    from tests.h2_helpers import PREFACE, frame, grpc_msg
    from tests.h2_hpack_lib import HH, headers_frames, literal
    from tests.h2_links_hpack_lib import _step
    from tests.h2_links_meta_lib import MH
    from tests.h2_links_meta_lib import compare as compare_meta
    from tests.h2_links_meta_lib import prepare as prepare_meta
    from tests.h2_meta_lib import request as header_list
    paths = (b"/svc/Unary", b"/svc/Stream")
    hhs, m, hs = [HH(gpu, prefix=True) for _ in range(3)], MH(gpu, methods=paths, accept=("identity", "gzip")), [CH(gpu, 16, 2) for _ in range(3)]
    arenas = [gpu.DeviceBuffer(nbytes=1 << 16) for _ in range(3)]
    asms = [h2dev.Assembler(hhs[i].parser, arenas[i], max_message_bytes=4096, max_pending=256) for i in range(3)]
    block = lambda hl: b"".join(literal(n, v, 2) for n, v in hl)  # noqa: E731
    wires = {i: PREFACE + frame(4, 0, 0) for i in range(3)}
    for s in (1, 3, 5):  # link 0: unary requests, one message each, END_STREAM
        wires[0] += headers_frames(s, block(header_list(paths[0], grpc_timeout=b"1S"))) + frame(0, 1, s, grpc_msg(b"u%d" % s * s))
    wires[1] += headers_frames(7, block(header_list(b"/svc/none"))) + frame(0, 0, 7, grpc_msg(b"lost"))  # link 1: refused, its message an orphan
    wires[2] += headers_frames(9, block(header_list(paths[1], grpc_encoding=b"gzip")))  # link 2: a stream of three messages
    wires[2] += frame(0, 0, 9, grpc_msg(b"a" * 300, 1) + grpc_msg(b"b")) + frame(0, 0, 9, grpc_msg(b"c" * 70))
    order, now = [2, 0, 1], 10**9
    # 1. deframe + assemble every link: the counts stand in last_call
    msgs, last = {}, {}
    for i in order:
        slices = [wires[i][:40], wires[i][40:]]
        hhs[i].buf, table = hhs[i].pp.upload(slices)
        hhs[i].last, hhs[i].last_slices = hhs[i].pp.expect(slices), slices
        err, msgs[i] = hhs[i].parser.deframe_messages(hhs[i].buf.ptr, table, asms[i], ev_cap=4096)
        assert err == 0
        last[i] = asms[i].last_call()
    assert [last[i][1] for i in range(3)] == [3, 1, 3]
    # 2. decode every link, 3. read every link where the decoders left it, 4. route: no table passes through the host
    decoded = _step(hhs, order, None, ())
    _, dgot = h2dev.decode_batch([(hhs[i].dec,) + hhs[i].target.args() for i in order])
    device = {}
    for k, i in enumerate(order):
        blocks, fields, strings, res = decoded[i]
        t = hhs[i].target
        device[i] = ((t.blocks.ptr, dgot[k][0], t.fields.ptr, dgot[k][1], t.strings.ptr, dgot[k][2]), ([tuple(b) for b in blocks], fields, strings))
    mitems, mlinks = prepare_meta(m, order, device=device)
    mcount, mgot = m.dev.read_batch(mitems)
    outs = {i: Out(gpu, 16, 16, 2) for i in order}
    items = [(hs[i].dev, hhs[i].target.blocks.ptr, mlinks[i].out.meta.ptr, mgot[k][0]) + tuple(last[i]) + (now,) + outs[i].args() for k, i in enumerate(order)]
    count, got = h2dev.calls_step_batch(items)
    # (the comparisons, behind the four calls; the models are fed with the device's own downloaded tables)
    compare_meta(m, order, mlinks, mcount, mgot)
    links = {}
    for i in order:
        mp, nmsgs, ep, nev = last[i]
        d_msgs = [struct.unpack("<QQQIIII", device_bytes(gpu, mp + 40 * j, 40))[:6] for j in range(nmsgs)]
        d_events = [struct.unpack("<6I", device_bytes(gpu, ep + 24 * j, 24)) for j in range(nev)]
        links[i] = Link(None, outs[i], hs[i].model.step([tuple(b) for b in decoded[i][0]], mlinks[i].exp[0], d_msgs, d_events, now, 16, 16))
    out = compare(hs, order, links, count, got)
    assert count == 3 and [out[i][3][:3] for i in range(3)] == [(3, 3, 0), (0, 0, 1), (1, 3, 0)]
    assert [out[i][1] for i in range(3)] == [[0, 3, 3, 3], [0, 0, 0, 1], [0, 0, 3, 3]] and reason(out[1][0][0]) == NO_CALL
    assert [(r[3], r[7], r[6] & 7) for r in out[0][0]] == [(1, 0, FIRST | LAST), (3, 0, FIRST | LAST), (5, 0, FIRST | LAST)]
    assert [(r[3], r[7], r[6] & 7) for r in out[2][0]] == [(9, 0, FIRST | COMPRESSED), (9, 1, 0), (9, 2, 0)]
    assert [bytes(asms[2].view(msgs[2][r[4]])) for r in out[2][0]] == [b"a" * 300, b"b", b"c" * 70]
    assert [(d[2], d[5]) for d in out[0][2]] == [(1, READS_CLOSED), (3, READS_CLOSED), (5, READS_CLOSED)]
    for a in asms:
        a.close()
    for x in hs + [m] + hhs:
        x.close()


# ---- refusals and lifetime ---------------------------------------------------------------------------------------------------------------
def test_refusals_and_lifetime(gpu):
    import ctypes as C

    import numpy as np
    from grpc_rdma_amd import h2dev
    from tests.h2_device_lib import same
    lib = h2dev.load()
    hs = [CH(gpu, 16, 3) for _ in range(3)]
    count, _, _ = step_batch(hs, range(3), steps={i: small(i) for i in range(3)})
    assert count == 3
    t = Tables(gpu, *zip(request(sid(50))), [message(sid(50))], [closed(sid(50), False)])
    links = {i: Link(None, Out(gpu, 4, 4, 3), None) for i in range(3)}
    items = [(hs[i].dev,) + t.args() + (0,) + links[i].out.args() for i in range(3)]
    bp, mp, nb, gp, ng, ep, ne = t.args()
    dp, dc, sp, fp, fc = links[1].out.args()

    def with_item(*rest):
        return [items[0], (hs[1].dev,) + rest, items[2]]

    gone = h2dev.CallTable(16, 2)
    gone.close()
    cases = [("none", [], "BATCH_MAX"), ("257 items", [items[0]] * 257, "BATCH_MAX"), ("the same table twice", [items[0], items[1], items[0]], "twice"),
             ("an item without table", [items[0], (None,) + items[1][1:]], "no table"), ("a closed table", [items[0], (gone,) + items[1][1:]], "no table"),
             ("no dispatch table", with_item(*t.args(), 0, 0, dc, sp, fp, fc), "null, zero or misaligned"),
             ("a zero dispatch cap", with_item(*t.args(), 0, dp, 0, sp, fp, fc), "null, zero or misaligned"),
             ("no segment table", with_item(*t.args(), 0, dp, dc, 0, fp, fc), "null, zero or misaligned"),
             ("no done list", with_item(*t.args(), 0, dp, dc, sp, 0, fc), "null, zero or misaligned"),
             ("a zero done cap", with_item(*t.args(), 0, dp, dc, sp, fp, 0), "null, zero or misaligned"),
             ("a misaligned dispatch table", with_item(*t.args(), 0, dp + 8, dc, sp, fp, fc), "null, zero or misaligned"),
             ("a misaligned segment table", with_item(*t.args(), 0, dp, dc, sp + 4, fp, fc), "null, zero or misaligned"),
             ("a misaligned done list", with_item(*t.args(), 0, dp, dc, sp, fp + 8, fc), "null, zero or misaligned"),
             ("no block table, one record", with_item(0, mp, nb, gp, ng, ep, ne, 0, dp, dc, sp, fp, fc), "null input table"),
             ("no record table, one record", with_item(bp, 0, nb, gp, ng, ep, ne, 0, dp, dc, sp, fp, fc), "null input table"),
             ("no descriptors, one message", with_item(bp, mp, nb, 0, ng, ep, ne, 0, dp, dc, sp, fp, fc), "null input table"),
             ("no events, one event", with_item(bp, mp, nb, gp, ng, 0, ne, 0, dp, dc, sp, fp, fc), "null input table"),
             ("2^20 + 1 descriptors", with_item(bp, mp, nb, gp, (1 << 20) + 1, ep, ne, 0, dp, dc, sp, fp, fc), "2^20"),
             ("2^32 - 1 records", with_item(bp, mp, 0xffffffff, gp, ng, ep, ne, 0, dp, dc, sp, fp, fc), "2^32 - 1"),
             ("2^32 - 1 events", with_item(bp, mp, nb, gp, ng, ep, 0xffffffff, 0, dp, dc, sp, fp, fc), "2^32 - 1"),
             ("no item array", None, "no item array"), ("no result array", None, "no result array")]
    for what, its, why in cases:
        if its is None:
            arr, out = np.array([(hs[0].dev.h,) + items[0][1:]], dtype="<u8"), (C.c_uint64 * 8)(*([7] * 8))
            args = (None, 1, out) if what == "no item array" else (arr.ctypes.data_as(C.c_void_p), 1, None)
            same(lib.grdma_h2_calls_step_batch(*args), INVALID, what)
            same(list(out), [7] * 8, what + ": the result words are not touched")
        else:
            with pytest.raises(gpu.GrdmaError, match=ERR2):
                h2dev.calls_step_batch(its)
            same([it[0].last_result for it in its if it[0] is not None], [(0,) * 8] * sum(1 for it in its if it[0] is not None),
                 what + ": the result words are not touched")
        assert why in lib.grdma_last_error().decode(), (what, lib.grdma_last_error())
        unchanged(hs, links, what)
    # nothing ran, nothing changed: the next batch is exact
    count, out, _ = step_batch(hs, [1, 0, 2], steps={i: small(3 + i) for i in range(3)})
    assert count == 3 and [h.dev.stats()["steps"] for h in hs] == [2, 2, 2]
    # close() directly behind a batch: the targets hold what the call wrote; the others go on
    x = [CH(gpu, 16, 3) for _ in range(2)]
    its, lk = prepare(x, [0, 1], steps={0: dict(reqs=[request(sid(k)) for k in range(8)], msgs=[message(sid(i % 9), length=i) for i in range(600)]), 1: small(1)})
    count, got = h2dev.calls_step_batch(its)
    close(x)
    compare(x, [0, 1], lk, count, got, tables=False)
    close(x)
    step_batch(hs, [2, 0], steps={0: small(7), 2: small(8)})
    close(hs)
