"""The call table on the device (grdma_h2_calls, csrc/grdma_h2_calls.h): per-call state keyed by stream, a step's
messages routed by method.  The expected values come from the CallsModel of tests/h2_calls_model.py: the rules of
include/grdma_amd.h ("Call table").  Every comparison is exact (CH of tests/h2_calls_lib.py runs a step on the device
and in the model and compares the dispatch table, the segment words and the done list whole -- what is not written
keeps its fill -- the result block, the dump and the counters); what a test asserts beside that is what the case is
about.  The tables are synthetic and uploaded directly; the shapes are the kernels' edges: the 64 lanes of a wave, the
256 descriptors a workgroup takes at a time, the run of a workgroup, the table's mask, the 4097 keys."""
import itertools

import pytest

from tests.h2_calls_lib import CH, Out, Tables, cluster_id
from tests.h2_calls_model import (BAD_INPUT, BAD_STATUS, COMPRESSED, COMPRESSED_IDENTITY, DEADLINE, ERR_METHOD, ERR_STREAM, EXPIRED_MSG,
                                  FIRST, LAST, LEFT, LOST, NO_CALL, NONE, READS_CLOSED, WAS_READS_CLOSED, closed, message, request)
from tests.h2_hpenc_lib import ERR2

pytestmark = pytest.mark.gpu

THREADS, GRID, EMU_GRID = 256, 64, 2  # H2C_THREADS, H2C_GRID of csrc/grdma_h2_calls.h on the device and under the emulator
COUNTS = [0, 1, 63, 64, 65, 255, 256, 257, EMU_GRID * THREADS + 1, GRID * THREADS + 3]


def sid(k):
    return 2 * k + 1


def reason(rec):
    return rec[6] >> 8 & 0xff


# ---- counts -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", COUNTS)
def test_record_counts(gpu, n):
    h = CH(gpu, table_slots=65536, nmethods=3)
    # every third record no request, every fifth refused
    reqs = [request(sid(k), k % 3, kind=2 if k % 3 == 2 else 1, verdict=6 if k % 5 == 4 else 0) for k in range(n)]
    opened = sum(1 for k in range(n) if k % 3 != 2 and k % 5 != 4)
    disp, segs, done, res = h.step(reqs, [message(sid(k)) for k in range(0, n, 7)])
    assert res[0] == opened and res[5] == opened
    h.close()


@pytest.mark.parametrize("n", COUNTS)
def test_message_counts(gpu, n):
    h = CH(gpu, nmethods=5)
    h.step([request(sid(k), k % 5, encoding=k % 2) for k in range(10)])
    # ten calls and an unknown stream, interleaved
    disp, segs, done, res = h.step(msgs=[message(sid(i * 7 % 11), length=i, offset=256 * i, compressed=i % 4 == 1) for i in range(n)])
    assert res[1] + res[2] == n and segs[-1] == n
    h.close()


@pytest.mark.parametrize("n", COUNTS)
def test_event_counts(gpu, n):
    h = CH(gpu, table_slots=65536)
    calls = min(n, 300)
    h.step([request(sid(k)) for k in range(calls)])
    # reads closed then left for the first calls, other kinds and unknown streams between
    events = [(closed(sid(j // 2), j % 2) if j // 2 < calls else (7, 1, 0, sid(10**6 + j), 0, 0)) if j % 3 else (5, 0, 0, sid(j // 2), 0, 0)
              for j in range(n)]
    disp, segs, done, res = h.step(events=events)
    assert res[3] == len(done) and res[5] == calls - sum(1 for d in done if d[5] & 0xff == LEFT)
    h.close()


# ---- methods ----------------------------------------------------------------------------------------------------------------
def test_no_method_registered(gpu):
    h = CH(gpu, nmethods=0)
    disp, segs, done, res = h.step(msgs=[message(1), message(3, status=1)])
    assert segs == [0, 2] and [reason(r) for r in disp] == [NO_CALL, BAD_STATUS]
    t, o = Tables(gpu, *zip(request(1, 0)), [], []), Out(gpu, 1, 1, 0)
    with pytest.raises(gpu.GrdmaError, match=ERR2):  # (any method is out of range)
        h.dev.step(*t.args(), 0, *o.args())
    h.close()


@pytest.mark.parametrize("nmethods", [1, 4096])
def test_every_message_on_one_method(gpu, nmethods):
    h = CH(gpu, nmethods=nmethods)
    h.step([request(sid(k), nmethods - 1) for k in range(4)])
    disp, segs, done, res = h.step(msgs=[message(sid(i % 4), length=i) for i in range(300)])
    assert segs[nmethods - 1:] == [0, 300, 300] and [r[4] for r in disp] == list(range(300))
    h.close()


def test_one_message_on_each_of_4096_methods(gpu):
    h = CH(gpu, table_slots=16384, nmethods=4096)
    # the calls' methods run against the streams; the messages come in stream order
    disp, segs, done, res = h.step([request(sid(k), 4095 - k) for k in range(4096)], [message(sid(k), length=k) for k in range(4096)])
    assert segs == list(range(4097)) + [4096] and [r[3] for r in disp] == [sid(4095 - m) for m in range(4096)]
    h.close()


def test_everything_orphaned(gpu):
    h = CH(gpu, nmethods=2)
    disp, segs, done, res = h.step(msgs=[message(sid(i % 5), status=i % 4) for i in range(300)])
    assert segs == [0, 0, 0, 300] and res[1:3] == (0, 300)
    h.close()


# ---- the table ----------------------------------------------------------------------------------------------------------------
CLUSTER = [cluster_id(hm, k) for hm in (14, 15, 0, 1) for k in range(2)]  # eight ids, two on each of the homes 14, 15, 0, 1


def test_sixteen_slots_clustered_on_the_wrap(gpu):
    h = CH(gpu, table_slots=16, nmethods=2)
    disp, segs, done, res = h.step([request(s, i % 2) for i, s in enumerate(CLUSTER)], [message(s, length=s) for s in CLUSTER])
    assert res[0] == 8 and res[1] == 8 and not res[6]
    # one more is lost; the others go on
    disp, segs, done, res = h.step([request(cluster_id(14, 2))], [message(cluster_id(14, 2))] + [message(s) for s in CLUSTER])
    assert res[0] == 0 and res[6] == LOST and reason(disp[-1]) == NO_CALL and [r[7] for r in disp[:-1]] == [1] * 8
    # two leave, two others come
    h.step(events=[closed(CLUSTER[0], True), closed(CLUSTER[3], True)])
    h.step([request(cluster_id(14, 2)), request(cluster_id(15, 2))])
    disp, segs, done, res = h.step(msgs=[message(cluster_id(14, 2)), message(cluster_id(15, 2)), message(CLUSTER[0])])
    assert res[5] == 8 and res[6] == LOST and [reason(r) for r in disp] == [0, 0, NO_CALL]
    h.close()


@pytest.mark.parametrize("order", list(itertools.permutations(range(4))), ids=lambda o: "".join(map(str, o)))
def test_opens_and_lefts_interleaved_in_a_cluster(gpu, order):
    h = CH(gpu, table_slots=16)
    ids = [cluster_id(15, k) for k in range(4)]  # one home: the probes wrap from 15 to 0, 1, 2
    h.step([request(s) for s in ids])
    for k in order:  # one leaves, its successor on the same home comes, everyone gets a message
        new = cluster_id(15, 4 + k)
        h.step([request(new)], [message(s) for s in ids], [closed(ids[k], True)])
        ids[k] = new
    disp, segs, done, res = h.step(msgs=[message(s) for s in ids])
    assert res[1] == 4 and res[5] == 4
    h.close()


def test_exactly_half_the_slots_live_and_one_more(gpu):
    h = CH(gpu, table_slots=64)
    disp, segs, done, res = h.step([request(sid(k)) for k in range(32)])
    assert res[0] == 32 and res[6] == 0
    # the first of the step goes in once one has left -- but LEFT comes behind OPEN: lost
    disp, segs, done, res = h.step([request(sid(40)), request(sid(41))], events=[closed(sid(0), True)])
    assert res[0] == 0 and res[5] == 31 and res[6] == LOST
    disp, segs, done, res = h.step([request(sid(40)), request(sid(41)), request(sid(40))])
    assert res[0] == 1 and res[5] == 32 and res[6] == LOST and h.model.serial == 33  # (sticky; the lost took no serial)
    h.close()


# ---- sequences within a call ----------------------------------------------------------------------------------------------------
def test_one_stream_across_tiles_and_steps(gpu):
    h = CH(gpu, nmethods=2)
    h.step([request(1, 1), request(3, 0), request(5, 0)])
    # stream 1 at the lanes 0, 63, 64, 65, 127, 128, 255, 256, 257 and 600, the others' messages between
    at = (0, 63, 64, 65, 127, 128, 255, 256, 257, 600)
    msgs = [message(1 if i in at else 3 + 2 * (i % 2), length=i) for i in range(700)]
    disp, segs, done, res = h.step(msgs=msgs)
    mine = [r for r in disp if r[3] == 1]
    assert [r[4] for r in mine] == list(at) and [r[7] for r in mine] == list(range(10)) and mine[0][6] & FIRST and not mine[1][6] & FIRST
    # the next step continues the count; the close comes with it: LAST on the last one
    disp, segs, done, res = h.step(msgs=[message(1), message(3), message(1)], events=[closed(1, False)])
    assert [(r[7], r[6] & LAST) for r in disp if r[3] == 1] == [(10, 0), (11, LAST)] and not any(r[6] & LAST for r in disp if r[3] != 1)
    assert done == [(0, sum(at) + 16, 1, 1, 12, READS_CLOSED)]
    # the close in a later step: no LAST anywhere
    disp, segs, done, res = h.step(msgs=[message(3)])
    disp2, _, done, res = h.step(events=[closed(3, True)])
    assert not disp[0][6] & LAST and disp2 == [] and done[0][5] == LEFT
    h.close()


# ---- duplicates ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("a,b", [(0, 63), (64, 65), (255, 256)])
def test_a_request_twice_in_a_step(gpu, a, b):
    h = CH(gpu, nmethods=2)
    reqs = [request(sid(k + 10)) for k in range(300)]
    reqs[a], reqs[b] = request(5, 1, encoding=1), request(5, 0)  # the first wins: method 1, gzip
    disp, segs, done, res = h.step(reqs, [message(5, compressed=True)])
    assert res[0] == 299 and disp[0][5] == 1 and disp[0][6] == FIRST | COMPRESSED | 1 << 16 and disp[0][2] == a
    # ... and across steps: the entry stays what it was
    disp, segs, done, res = h.step([request(5, 0)], [message(5)])
    assert res[0] == 0 and (disp[0][5], disp[0][7]) == (1, 1)
    h.close()


# ---- step ordering and limits ---------------------------------------------------------------------------------------------------
def test_every_orphan_reason_in_the_order_of_the_checks(gpu):
    h = CH(gpu)
    h.step([request(1, timeout=5), request(3), request(5, encoding=1)], now=100)
    msgs = [message(7, status=2),                 # no call, and a bad status: the status is looked at first
            message(7),                           # no call
            message(1, status=3),                 # expired, and a bad status
            message(1, compressed=True),          # expired, and compressed on identity: expired
            message(3, compressed=True),          # compressed on identity
            message(5, compressed=True),          # gzip: dispatched
            message(3)]
    disp, segs, done, res = h.step(msgs=msgs, now=105)
    assert [(r[4], reason(r)) for r in disp] == [(5, 0), (6, 0), (0, BAD_STATUS), (1, NO_CALL), (2, BAD_STATUS), (3, EXPIRED_MSG),
                                                (4, COMPRESSED_IDENTITY)]
    assert done == [(0, 0, 1, 0, 0, DEADLINE)] and all(r[5] == NONE and r[7] == 0 for r in disp[2:])
    h.close()


def test_expiry_order_in_the_done_list(gpu):
    h = CH(gpu, table_slots=1024)
    streams = [sid(k * 37 % 301) for k in range(301)]  # opened in no order
    h.step([request(s, timeout=s) for s in streams], now=1000)
    h.step(events=[closed(sid(3), False)], now=1000)
    # the deadlines up to 1200 pass; two streams close in the same step: the deadlines first, by stream, then the closes
    disp, segs, done, res = h.step(events=[closed(sid(200), True), closed(sid(2), False)], now=1200, msgs=[message(sid(3)), message(sid(150))])
    dead = [d for d in done if d[5] & 0xff == DEADLINE]
    assert [d[2] for d in dead] == sorted(s for s in streams if s <= 200) and res[4] == len(dead) == 100
    assert [d[5] for d in dead if d[2] == sid(3)] == [DEADLINE | WAS_READS_CLOSED << 8]
    assert [(d[2], d[5]) for d in done[100:]] == [(sid(200), LEFT), (sid(2), READS_CLOSED)]
    assert [reason(r) for r in disp] == [0, EXPIRED_MSG]
    # timeout 0 expires in the step that opens it; a second pass of the same clock expires nothing again
    disp, segs, done, res = h.step([request(sid(500), timeout=0)], [message(sid(500))], now=1200)
    assert done == [(301, 0, sid(500), 0, 0, DEADLINE)] and reason(disp[0]) == EXPIRED_MSG
    h.close()


def test_reads_closed_then_left(gpu):
    h = CH(gpu)
    h.step([request(1), request(3), request(5)], [message(1, length=10), message(3, length=20)])
    disp, segs, done, res = h.step(events=[closed(1, False), closed(1, True), closed(3, True), closed(3, False), closed(5, False), closed(5, False)])
    assert done == [(0, 10, 1, 0, 1, READS_CLOSED), (0, 10, 1, 0, 1, LEFT | WAS_READS_CLOSED << 8), (1, 20, 3, 0, 1, LEFT),
                    (2, 0, 5, 0, 0, READS_CLOSED), (2, 0, 5, 0, 0, READS_CLOSED)] and res[5] == 1
    h.close()


@pytest.mark.parametrize("short", ["dispatch", "done"])
def test_a_cap_too_small_writes_nothing_and_the_repeat_is_exact(gpu, short):
    h = CH(gpu, table_slots=16, nmethods=2)
    h.step([request(sid(k)) for k in range(7)])
    reqs = [request(sid(7), 1, timeout=0), request(sid(8), 1)]  # (the second would be lost)
    msgs = [message(sid(k)) for k in range(9)]
    events = [closed(sid(0), True), closed(sid(1), False)]
    caps = dict(dispatch_cap=8, done_cap=8) if short == "dispatch" else dict(dispatch_cap=16, done_cap=2)
    disp, segs, done, res = h.step(reqs, msgs, events, now=5, **caps)
    assert res[7] == 1 and res[:7] == (1, 7, 2, 3, 1, 7, LOST) and disp == [] and h.model.lost == 0
    disp, segs, done, res = h.step(reqs, msgs, events, now=5)
    assert res == (1, 7, 2, 3, 1, 7, LOST, 0) and len(disp) == 9
    h.close()


def test_bad_input_names_the_record(gpu):
    h = CH(gpu, nmethods=2)
    good = [request(sid(k)) for k in range(300)]
    for at, bad, code in ((299, request(0), ERR_STREAM), (64, request(1 << 31), ERR_STREAM), (0, request(9, 2), ERR_METHOD),
                          (257, request(0, 7), ERR_STREAM)):
        reqs = list(good)
        reqs[at] = bad
        if at == 64:
            reqs[200] = request(11, 5)  # (a second one behind it: the first is reported)
        disp, segs, done, res = h.step(reqs, [message(1)])
        assert res == (0, 0, 0, 0, 0, 0, BAD_INPUT | code << 8 | at << 32, 0)
    # what cannot open a call is not looked at
    disp, segs, done, res = h.step([request(0, 9, verdict=1), request(0, 9, kind=3), request(0, 9, status=1)] + good)
    assert res[0] == 300 and h.dev.stats()["steps"] == 1  # (not sticky, and a refused step counts nowhere)
    h.close()


def test_refusals_and_lifetime(gpu):
    from grpc_rdma_amd import h2dev
    lib = h2dev.load()
    for args in ((8, 1), (24, 1), (1 << 17, 1), (16, 4097)):
        assert not lib.grdma_h2_calls_create(*args) and lib.grdma_last_error()
    with pytest.raises(gpu.GrdmaError):
        h2dev.CallTable(17, 0)
    h = CH(gpu)
    t = Tables(gpu, *zip(request(1)), [message(1)], [closed(1, False)])
    o = Out(gpu, 4, 4, 1)
    dp, dc, sp, fp, fc = o.args()
    for targets in ((0, dc, sp, fp, fc), (dp, 0, sp, fp, fc), (dp, dc, 0, fp, fc), (dp, dc, sp, 0, fc), (dp, dc, sp, fp, 0), (dp + 8, dc, sp, fp, fc),
                    (dp, dc, sp + 4, fp, fc), (dp, dc, sp, fp + 8, fc)):
        with pytest.raises(gpu.GrdmaError, match=ERR2):
            h.dev.step(*t.args(), 0, *targets)
    bp, mp, nb, gp, ng, ep, ne = t.args()
    for tables in ((0, mp, nb, gp, ng, ep, ne), (bp, 0, nb, gp, ng, ep, ne), (bp, mp, nb, 0, ng, ep, ne), (bp, mp, nb, gp, ng, 0, ne),
                   (bp, mp, nb, gp, (1 << 20) + 1, ep, ne), (bp, mp, 0xffffffff, gp, ng, ep, ne), (bp, mp, nb, gp, ng, ep, 0xffffffff)):
        with pytest.raises(gpu.GrdmaError, match=ERR2):
            h.dev.step(*tables, 0, dp, dc, sp, fp, fc)
    assert lib.grdma_h2_calls_step(h.dev.h, bp, mp, nb, gp, ng, ep, ne, 0, dp, dc, sp, fp, fc, None) == -2  # no result array
    assert lib.grdma_h2_calls_step(None, bp, mp, nb, gp, ng, ep, ne, 0, dp, dc, sp, fp, fc, None) == -2     # no table
    assert o.dispatch.read() == bytes([0xA5]) * (48 * 6) and o.done.read() == bytes([0xA5]) * (32 * 6) and o.segments.read() == bytes([0xA5]) * 28
    h.step([request(1)], [message(1)], [closed(1, False)])  # nothing of that changed anything
    other = CH(gpu, table_slots=16, nmethods=3)  # a second table beside the first
    other.step([request(1, 2)], [message(1)])
    h.close()
    h.close()
    other.step(msgs=[message(1)])
    other.close()
    for _ in range(3):  # create and destroy with a step in between
        x = CH(gpu)
        x.step([request(1)], [message(1)])
        x.close()


# ---- the chain on device tables ---------------------------------------------------------------------------------------------------
def test_deframe_decode_read_and_route_on_device_tables(gpu):
    import struct
    from grpc_rdma_amd import h2dev
    from tests.h2_helpers import PREFACE, frame, grpc_msg
    from tests.h2_hpack_lib import HH, headers_frames, literal
    from tests.h2_meta_lib import MH, request as header_list
    paths = (b"/svc/Unary", b"/svc/Stream")
    hh, m = HH(gpu, prefix=True), MH(gpu, methods=paths, accept=("identity", "gzip"))
    h = CH(gpu, nmethods=2)
    arena = gpu.DeviceBuffer(nbytes=1 << 16)
    asm = h2dev.Assembler(hh.parser, arena, max_message_bytes=4096, max_pending=256)
    block = lambda hs: b"".join(literal(n, v, 2) for n, v in hs)  # noqa: E731
    wire = PREFACE + frame(4, 0, 0)
    for s in (1, 3, 5):  # unary requests: one message, END_STREAM
        wire += headers_frames(s, block(header_list(paths[0], grpc_timeout=b"1S"))) + frame(0, 1, s, grpc_msg(b"u%d" % s * s))
    wire += headers_frames(7, block(header_list(b"/svc/none")))  # refused: its message is an orphan
    wire += headers_frames(9, block(header_list(paths[1], grpc_encoding=b"gzip")))
    wire += frame(0, 0, 7, grpc_msg(b"lost")) + frame(0, 0, 9, grpc_msg(b"a" * 300, 1) + grpc_msg(b"b")) + frame(0, 0, 9, grpc_msg(b"c" * 70))
    slices = [wire[:40], wire[40:]]
    # deframe + assemble, decode, read: on the stream of the calls; the reads below are the test's comparisons
    buf, table = hh.pp.upload(slices)
    hh.last, hh.last_slices = hh.pp.expect(slices), slices
    err, msgs = hh.parser.deframe_messages(buf.ptr, table, asm, ev_cap=4096)
    assert err == 0 and len(msgs) == 7
    mp, nmsgs, ep, nev = asm.last_call()
    assert nmsgs == 7 and nev == len(hh.last[1])
    blocks, dres = hh.decode()
    t = hh.target
    words = lambda data, n: [tuple(int.from_bytes(data[16 * i + 4 * j:16 * i + 4 * j + 4], "little") for j in range(4)) for i in range(n)]  # noqa: E731
    raw = tuple(x.read() for x in (t.blocks, t.fields, t.strings))
    recs, rej, mres = m.read(raw=(words(raw[0], dres[0]), words(raw[1], dres[1]), raw[2][:dres[2]]),
                             device=(t.blocks.ptr, dres[0], t.fields.ptr, dres[1], t.strings.ptr, dres[2]))
    # the model is fed with the device's own downloaded tables
    from tests.h2_device_lib import device_bytes
    d_msgs = [struct.unpack("<QQQIIII", device_bytes(gpu, mp + 40 * i, 40))[:6] for i in range(nmsgs)]
    d_events = [struct.unpack("<6I", device_bytes(gpu, ep + 24 * i, 24)) for i in range(nev)]
    reqs = list(zip(words(raw[0], dres[0]), recs))
    disp, segs, done, res = h.step(reqs, d_msgs, d_events, now=10**9,
                                   device=(t.blocks.ptr, m.last_out.meta.ptr, dres[0], mp, nmsgs, ep, nev))
    assert res[:3] == (4, 6, 1) and segs == [0, 3, 6, 7]
    assert [(r[3], r[7], r[6] & 7) for r in disp] == [(1, 0, FIRST | LAST), (3, 0, FIRST | LAST), (5, 0, FIRST | LAST), (9, 0, FIRST | COMPRESSED),
                                                     (9, 1, 0), (9, 2, 0), (7, 0, 0)]
    assert [bytes(asm.view(msgs[r[4]])) for r in disp[3:6]] == [b"a" * 300, b"b", b"c" * 70] and reason(disp[6]) == NO_CALL
    assert [(d[2], d[5]) for d in done] == [(1, READS_CLOSED), (3, READS_CLOSED), (5, READS_CLOSED)]
    asm.close()
    for x in (h, m, hh):
        x.close()
