"""The stream-keyed state of the HTTP/2 receive path under colliding and crowded stream ids: the parser's stream map
(tab_find / tab_insert / tab_remove, csrc/grdma_h2_kernels.h), the assembler's carry table (h2a_tab_*,
csrc/grdma_h2_asm.h), the LDS hash and the keyed wave scans of the assembler's plan (csrc/grdma_h2_asm_stage.inc) and
the ledger's scratch table (h2fc_claim / h2fc_find, csrc/grdma_h2_fc.h).  All four hash a stream to (id >> 1) & mask
and probe linearly; the first two delete by backward shift.

With table_slots=16 the mask is 15 and stream 2 * (h + 16 k) + 1 has home h: the ids below sit in clusters on homes
14, 15, 0 and 1, so probing and shifting cross the end of the table.  References: the CPU oracle (pyorc.H2Parser), the
sequential assembler model (tests/h2_asm_model.py) and the ledger's model (tests/h2_flow_model.py, here with the
slot rule of rule 4).  Every comparison is exact."""
import itertools
import random

import pytest

from oracle.pyorc import EV_FRAME, EV_STREAM_CLOSED, EV_STREAM_OPEN
from tests.h2_asm_model import OK, TRUNCATED
from tests.h2_device_lib import ERR_CAPACITY, FH, SENTINEL, Conn, Harness, cut_mean, fast_sender_slices, pack_slices
from tests.h2_flow_model import LOST, STREAM, Model
from tests.h2_helpers import PREFACE, frame, grpc_msg

pytestmark = pytest.mark.gpu

SLOTS = 16
WRAP8 = (29, 31, 33, 61, 63, 65, 93, 95)         # homes 14 15 0 14 15 0 14 15 -> slots 14 15 0 1 2 3 4 5
HOME0 = tuple(32 * k + 1 for k in range(8))      # 1, 33, 65, ...: all on home 0, one cluster of eight
WRAP4 = (31, 33, 63, 65)                         # homes 15 0 15 0 -> slots 15 0 1 2
POOL24 = tuple(2 * (h + 16 * k) + 1 for k in range(6) for h in (14, 15, 0, 1))
ERR_MAX_STREAMS = 9
RST = (8).to_bytes(4, "big")
assert [(s >> 1) & 15 for s in WRAP8] == [14, 15, 0, 14, 15, 0, 14, 15] and all((s >> 1) & 15 == 0 for s in HOME0)
assert [(s >> 1) & 15 for s in WRAP4] == [15, 0, 15, 0] and {(s >> 1) & 15 for s in POOL24} == {14, 15, 0, 1}


class Src:
    """what one stream sends: gRPC messages back to back, taken a few bytes at a time"""

    def __init__(self, rng, lens):
        self.msgs = [bytes(rng.getrandbits(8) for _ in range(n)) for n in lens]
        self.wire = b"".join(grpc_msg(m) for m in self.msgs)
        self.pos = 0

    def take(self, n):
        part = self.wire[self.pos:self.pos + n]
        self.pos += len(part)
        return part

    def rest(self):
        return self.take(len(self.wire))

    def complete(self):
        """the messages whose last byte has been taken"""
        out, end = [], 0
        for m in self.msgs:
            end += 5 + len(m)
            if end <= self.pos:
                out.append(m)
        return out


# ---- 1a. the parser's map: removal orders across the wrap ---------------------------------------------------------
FIRST = [3, 1, 5, 6, 40, 2, 17, 9]   # bytes of the message sent before the first removal: inside the 5-byte header too


def _removal_run(g, ids, order, n_rst, seed):
    """a server connection opens `ids`, leaves every one mid-message, removes order[:n_rst] with RST_STREAM one per
    call while the others go on a few bytes at a time, completes the rest and removes them through close_writes"""
    rng = random.Random(seed)
    src = {s: Src(rng, [rng.randrange(120, 300)]) for s in ids}
    calls = [[PREFACE + frame(4, 0, 0)] + [frame(1, 4, s, b"\x82\x86") for s in ids] +
             [frame(0, 0, s, src[s].take(FIRST[i])) for i, s in enumerate(ids)]]
    left = list(ids)
    for r in order[:n_rst]:
        left.remove(r)
        fr = [frame(0, 0, left[0], src[left[0]].take(rng.randrange(1, 7))), frame(3, 0, r, RST)]
        fr += [frame(0, 0, s, src[s].take(rng.randrange(1, 7))) for s in left]
        fr.append(frame(0, 0, r, b"late"))           # the removed id: skipped
        calls.append(fr)
    calls.append([frame(0, 0, s, src[s].take(rng.randrange(1, 7))) for s in left] +
                 [frame(0, 1, s, src[s].rest()) for s in left])
    # a call ends inside the frame header of the next call's first frame (always a DATA frame), or right behind it
    data = [b"".join(c) for c in calls]
    for i in range(len(data) - 1):
        sh = 4 if i == 0 else rng.choice([0, 4, 9, 2])
        data[i], data[i + 1] = data[i] + data[i + 1][:sh], data[i + 1][sh:]
    c = Conn(g, True)
    for d in data:
        c.call(cut_mean(d, rng))
    assert c.live() == len(left)
    assert sorted(c.done) == sorted((s, src[s].msgs[0]) for s in left) and not c.partial
    for s in order[n_rst:]:
        c.close_writes([s])
        c.call(cut_mean(b"".join(frame(0, 0, t, b"gone") for t in ids), rng))
    assert c.live() == 0 and len(c.done) == len(left)
    c.close()


def test_parser_map_every_removal_order_of_a_cluster_over_the_wrap(gpu):
    for k, order in enumerate(itertools.permutations(WRAP4)):
        _removal_run(gpu, WRAP4, order, 3, k)


@pytest.mark.parametrize("group", range(5))
def test_parser_map_random_removal_orders_of_eight(gpu, group):
    """ten seeded orders per case, fifty in all"""
    for seed in range(10 * group, 10 * group + 10):
        order = list(WRAP8)
        random.Random(1000 + seed).shuffle(order)
        _removal_run(gpu, WRAP8, order, 6, seed)


def test_parser_map_removal_orders_of_one_long_cluster(gpu):
    """all eight streams on home 0"""
    for seed in range(10):
        order = list(HOME0)
        random.Random(2000 + seed).shuffle(order)
        _removal_run(gpu, HOME0, order, 6, seed)


# ---- 1b. client side, random operations ----------------------------------------------------------------------------
def _client_sequence(g, seed, steps=25):
    rng = random.Random(seed)
    c = Conn(g, False)
    st = {}            # id -> dict(src, reads, writes) while the id is in the map
    expected = {s: [] for s in POOL24}

    def leave(s):
        expected[s] += st.pop(s)["src"].complete()

    def reads_closed(s):
        if st[s]["reads"]:
            st[s]["reads"] = False
            expected[s] += st[s]["src"].complete()
            st[s]["src"] = Src(rng, [])
        if not st[s]["writes"]:
            leave(s)

    for step in range(steps):
        readable = [s for s in st if st[s]["reads"]]
        op = rng.choice(["open", "open", "data", "data", "data", "end", "closew", "rst", "junk"])
        if op == "open" or not st:
            free = [s for s in POOL24 if s not in st]
            s = rng.choice(free)
            if len(st) < SLOTS // 2:
                c.open([s])
                st[s] = dict(src=Src(rng, [rng.choice([0, 1, 7, 40]) for _ in range(40)]), reads=True, writes=True)
            else:
                assert c.dev.open_streams([s]) == 1   # (the half-full rule: the ninth is refused)
                c.live()
            continue
        if op == "closew":
            cand = [s for s in st if st[s]["writes"]]
            if cand:
                s = rng.choice(cand)
                c.close_writes([s])
                st[s]["writes"] = False
                if not st[s]["reads"]:
                    leave(s)
                continue
            op = "data"
        frames = []
        if op == "junk":
            s = rng.choice([t for t in POOL24 if t not in st or not st[t]["reads"]])
            frames.append(frame(0, 0, s, b"skipped"))
        elif op == "rst":
            s = rng.choice(list(st))
            frames.append(frame(3, 0, s, RST))
            leave(s)
        elif op == "end" and readable:
            s = rng.choice(readable)
            if rng.randrange(2):
                frames.append(frame(0, 1, s, st[s]["src"].take(rng.randrange(0, 11))))
            else:
                frames.append(frame(1, 5, s, b"\x88"))
            reads_closed(s)
        # ... and DATA cut mid-message on up to two readable streams
        for s in rng.sample(sorted(t for t in st if st[t]["reads"]), min(2, len([t for t in st if st[t]["reads"]]))):
            frames.append(frame(0, 0, s, st[s]["src"].take(rng.randrange(1, 31))))
        if frames:
            c.call(cut_mean(b"".join(frames), rng, 12))
    for s in list(st):
        leave(s)
    got = {s: [] for s in POOL24}
    for s, m in c.done:
        got[s].append(m)
    assert got == expected
    c.close()


@pytest.mark.parametrize("group", range(10))
def test_parser_map_client_random_operations(gpu, group):
    """ten seeded sequences of 25 operations per case, a hundred in all"""
    for seed in range(10 * group, 10 * group + 10):
        _client_sequence(gpu, 3000 + seed)


# ---- 1c. the half-full rule ------------------------------------------------------------------------------------------
def test_parser_map_half_full_rule(gpu):
    rng = random.Random(1)
    nine = WRAP8 + (97,)
    # server: the ninth concurrent stream fails the connection
    c = Conn(gpu, True)
    c.call(cut_mean(PREFACE + frame(4, 0, 0) + b"".join(frame(1, 4, s, b"\x82") for s in nine), rng), want_err=ERR_MAX_STREAMS)
    assert c.dev.live_streams() == 8
    c.close()
    # client: the ninth id is refused, the eight before it stay usable
    c = Conn(gpu, False)
    assert c.dev.open_streams(nine) == 1
    for s in WRAP8:
        assert c.orc.open_stream(s) == 0
    assert c.live() == 8
    body = {s: bytes([s]) * (s % 50) for s in nine}
    c.call(cut_mean(b"".join(frame(0, 0, s, grpc_msg(body[s])) for s in nine), rng))
    assert c.done == [(s, body[s]) for s in WRAP8]
    c.close()


# ---- 1d. one chunked call on a stream that does not sit in its home slot, then on the shifted entry ------------------
def test_parser_map_chunked_call_on_a_shifted_entry(gpu):
    c = Conn(gpu, False, boundary_step=True)
    c.open([1, 33])                                   # both on home 0: 33 sits in slot 1
    c.call([frame(0, 1, 1, grpc_msg(b"first"))] + fast_sender_slices([3072] * 3, sid=33, max_frame=1024))
    assert c.dev.chunk_stats() == (0, 0)              # (too short, and no hint before it)
    body = fast_sender_slices([3072] * 300, sid=33, seed=1, max_frame=1024)
    assert len(body) >= 2048
    c.call(body)
    assert c.dev.chunk_stats() == (1, 1)              # the map is what the hint was recorded in: planned and merged
    c.close_writes([1])                               # 1 leaves the map: 33 moves back into slot 0
    assert c.live() == 1
    c.call(fast_sender_slices([3072] * 300, sid=33, seed=2, max_frame=1024))
    moved = c.dev.chunk_stats()
    c.call(fast_sender_slices([3072] * 300, sid=33, seed=3, max_frame=1024))
    print("chunked calls (planned, merged) after the streaming entry moved: %r, one call later %r" % (moved, c.dev.chunk_stats()))
    assert len(c.done) == 1 + 3 + 900 and all(s == 33 and len(m) == 3072 for s, m in c.done[1:])
    c.close()


# ---- 2a. the assembler's carry table ---------------------------------------------------------------------------------
def _carry_run(g, ids, order, n_removed, seed):
    """messages partial over several calls on every colliding stream; order[:n_removed] are cut off mid-message (RST_STREAM
    and END_STREAM in turn: TRUNCATED, the carry entry deleted with a backward shift) while the others go on; a freed id
    is opened again and starts a new message; the rest completes"""
    rng = random.Random(seed)
    h = Harness(g, 64 << 10, streams=list(ids), table_slots=SLOTS)
    src = {s: Src(rng, [rng.randrange(300, 900)]) for s in ids}
    for call in range(rng.randrange(2, 4)):          # with the removal calls: partial over 3 to 5 calls and more
        got = h.feed(cut_mean(b"".join(frame(0, 0, s, src[s].take(FIRST[(i + call) % 8] + 5 * call)) for i, s in enumerate(ids)), rng))
        assert got == []
    left, reopened = list(ids), None
    for n, r in enumerate(order[:n_removed]):
        left.remove(r)
        fr = [frame(0, 0, left[0], src[left[0]].take(rng.randrange(1, 30)))]
        fr.append(frame(3, 0, r, RST) if n % 2 == 0 else frame(0, 1, r, src[r].take(rng.randrange(0, 9))))
        fr += [frame(0, 0, s, src[s].take(rng.randrange(1, 30))) for s in left]
        got = h.feed(cut_mean(b"".join(fr), rng))
        assert [(m.stream_id, m.status) for m in got] == [(r, TRUNCATED)]
        if n == 0:
            # the id RST_STREAM freed starts a new call with a new message, partial as the others are
            h.pp.open([r])
            reopened = r
            src[r] = Src(rng, [rng.randrange(300, 900)])
            left.append(r)
            assert h.feed(cut_mean(frame(0, 0, r, src[r].take(rng.randrange(1, 200))), rng)) == []
    got = h.feed(cut_mean(b"".join(frame(0, 0, s, src[s].rest()) for s in left), rng))
    assert [(m.stream_id, m.status) for m in got] == [(s, OK) for s in left] and reopened in left
    assert [h.asm.view(m) for m in got] == [src[s].msgs[0] for s in left]
    h.release()
    assert h.asm.stats()["bytes_in_use"] == h.model.bytes_in_use() == 0
    h.close()


def test_carry_table_every_removal_order_of_a_cluster_over_the_wrap(gpu):
    for k, order in enumerate(itertools.permutations(WRAP4)):
        _carry_run(gpu, WRAP4, order, 3, k)


@pytest.mark.parametrize("group", range(5))
def test_carry_table_random_removal_orders_of_eight(gpu, group):
    """ten seeded orders per case, fifty in all; the odd seeds with all eight streams on home 0"""
    for seed in range(10 * group, 10 * group + 10):
        ids = HOME0 if seed % 2 else WRAP8
        order = list(ids)
        random.Random(4000 + seed).shuffle(order)
        _carry_run(gpu, ids, order, 5, seed)


# ---- 2b / 2c. crowded tiles, LDS hash collisions and wrap ------------------------------------------------------------
def _interleaved_messages(ids, rng, nmsg, shuffled):
    """every stream sends nmsg messages of 0 .. 200 bytes as 1 .. 4 DATA frames each; round-robin over the streams, or in
    a shuffled order -> (wire, {stream: [message, ...]})"""
    msgs = {s: [bytes(rng.getrandbits(8) for _ in range(rng.randrange(0, 201))) for _ in range(nmsg)] for s in ids}
    queue = {}
    for s in ids:
        q = []
        for m in msgs[s]:
            w = grpc_msg(m)
            k = min(rng.randrange(1, 5), len(w))
            cuts = [0] + sorted(rng.sample(range(1, len(w)), k - 1)) + [len(w)]
            q += [frame(0, 0, s, w[a:b]) for a, b in zip(cuts, cuts[1:])]
        queue[s] = q
    wire = bytearray()
    while any(queue.values()):
        if shuffled:
            s = rng.choice([t for t in ids if queue[t]])
            wire += queue[s].pop(0)
        else:
            for s in ids:
                if queue[s]:
                    wire += queue[s].pop(0)
    return bytes(wire), msgs


def _assemble(g, ids, slots, seed, shuffled, ncalls, arena=256 << 10):
    rng = random.Random(seed)
    wire, msgs = _interleaved_messages(ids, rng, 3, shuffled)
    bounds = [0] + sorted(rng.sample(range(1, len(wire)), ncalls - 1)) + [len(wire)]
    h = Harness(g, arena, streams=list(ids), table_slots=slots)
    got = []
    for a, b in zip(bounds, bounds[1:]):
        got += h.feed(cut_mean(wire[a:b], rng, 700))      # (descriptors and bytes against the model, call by call)
    by_stream = {s: [] for s in ids}
    for m in got:
        assert m.status == OK
        by_stream[m.stream_id].append(h.asm.view(m))
    assert by_stream == msgs
    h.close()


@pytest.mark.parametrize("ncalls", [1, 3])
@pytest.mark.parametrize("shuffled", [False, True], ids=["round_robin", "shuffled"])
def test_assembler_crowded_tiles(gpu, shuffled, ncalls):
    """96 streams: every 64-event tile holds up to 64 distinct keys, every stream's aggregate crosses tiles"""
    _assemble(gpu, tuple(range(1, 193, 2)), 256, 7 + ncalls, shuffled, ncalls)


LDS_IDS = (8191, 16383, 24575, 1, 8193, 16385, 3)   # LDS homes 4095 4095 4095 0 0 0 1: the probe wraps to slot 0


@pytest.mark.parametrize("ncalls", [1, 3])
@pytest.mark.parametrize("shuffled", [False, True], ids=["round_robin", "shuffled"])
@pytest.mark.parametrize("slots", [16, 4096])
def test_assembler_lds_hash_collisions_and_wrap(gpu, slots, shuffled, ncalls):
    assert [(s >> 1) & 4095 for s in LDS_IDS] == [4095, 4095, 4095, 0, 0, 0, 1]
    _assemble(gpu, LDS_IDS, slots, 11 + ncalls, shuffled, ncalls, arena=64 << 10)


# ---- 2d. the distinct-stream limit -----------------------------------------------------------------------------------
LIMIT = 3072


def _one_byte_messages(n):
    return b"".join(frame(0, 0, 2 * i + 1, grpc_msg(bytes([i % 251]))) for i in range(n))


def _failed_call(h, wire):
    """one call through the harness's parser and assembler that must fail with GRDMA_ERR_CAPACITY; the oracle's parser
    and the model are told"""
    data, table = pack_slices([wire])
    buf = h.g.DeviceBuffer(data=data)
    with pytest.raises(h.g.GrdmaError, match="error %d" % ERR_CAPACITY):
        h.parser.deframe_messages(buf.ptr, table, h.asm)
    h.pp.expect([wire])
    h.model.failed_call()


def test_assembler_exactly_the_stream_limit(gpu):
    h = Harness(gpu, 1 << 20, streams=list(range(1, 2 * LIMIT, 2)), table_slots=8192)
    got = h.feed([_one_byte_messages(LIMIT)])
    assert len(got) == LIMIT and all(m.status == OK for m in got)
    assert [m.stream_id for m in got] == list(range(1, 2 * LIMIT, 2)) and [m.seq for m in got] == list(range(LIMIT))
    h.close()


def test_assembler_one_stream_over_the_limit(gpu):
    """The contract of a call that fails on the stream limit (include/grdma_amd.h): nothing is assembled -- no
    descriptor, no arena byte, bytes in use, records and the seq counter as they were -- and the messages the streams
    carried into the call are dropped.  The next call is assembled as if the failed one had not been."""
    n = LIMIT + 1
    arena = 1 << 20
    h = Harness(gpu, arena, streams=list(range(1, 2 * n, 2)), table_slots=8192)
    first = h.feed([frame(0, 0, 5, grpc_msg(b"before")), frame(0, 0, 7, grpc_msg(b"partial" * 40)[:100])])
    assert [(m.stream_id, m.seq) for m in first] == [(5, 0)]
    image, in_use, st0 = h.arena.read(), h.asm.stats()["bytes_in_use"], h.asm.stats()
    assert in_use == 256 + 512 == h.model.bytes_in_use()
    _failed_call(h, _one_byte_messages(n))
    st = h.asm.stats()
    assert st["bytes_in_use"] == in_use and st["reported"] == st0["reported"] and st["ok_bytes"] == st0["ok_bytes"]
    assert h.arena.read() == image                    # no byte left its sentinel (or changed at all)
    # the rest of stream 7's message arrives: the message lost the failed call's bytes, so it is gone -- no descriptor
    # ever reports it, its space is free once the messages in front of it are released
    h.release()
    assert h.asm.stats()["bytes_in_use"] == h.model.bytes_in_use() == 0
    rest = grpc_msg(b"partial" * 40)[100:-6]       # (the deframer took the six bytes stream 7 sent in the failed call for it)
    got = h.feed([frame(0, 0, 7, rest), frame(0, 0, 9, grpc_msg(b"after")), frame(0, 0, 2 * n - 1, grpc_msg(b"z" * 300))])
    assert [(m.stream_id, m.seq, m.status, m.offset) for m in got] == [(9, 2, OK, 768), (2 * n - 1, 3, OK, 1024)]
    assert h.asm.stats()["bytes_in_use"] == h.model.bytes_in_use() == 256 + 512
    h.close()


def test_assembler_stream_limit_in_a_batch_of_two(gpu):
    """through grdma_h2_deframe_messages_batch: the item over the limit reports -GRDMA_ERR_CAPACITY, the other one is
    what its single call gives"""
    from grpc_rdma_amd import h2dev
    n = LIMIT + 1
    ok_wire = _one_byte_messages(200)
    single = Harness(gpu, 1 << 18, streams=list(range(1, 401, 2)), table_slots=8192)
    alone = single.feed([ok_wire])
    bytes_alone = single.arena.read()
    single.close()
    arenas = [gpu.DeviceBuffer(data=bytes([SENTINEL]) * (1 << 18)) for _ in range(2)]
    parsers = [h2dev.Parser(False, table_slots=8192) for _ in range(2)]
    assert parsers[0].open_streams(list(range(1, 2 * n, 2))) == 0 and parsers[1].open_streams(list(range(1, 401, 2))) == 0
    asms = [h2dev.Assembler(p, a, 4 << 20, 4096) for p, a in zip(parsers, arenas)]
    items, keep = [], []
    for p, a, wire in zip(parsers, asms, (_one_byte_messages(n), ok_wire)):
        data, table = pack_slices([wire])
        keep.append(gpu.DeviceBuffer(data=data))
        items.append((p, a, keep[-1].ptr, table))
    res = h2dev.deframe_messages_batch(items)
    assert res[0] == (0, -ERR_CAPACITY)
    assert res[1][0] == 0 and [tuple(m) for m in res[1][1]] == [tuple(m) for m in alone]
    assert arenas[0].read() == bytes([SENTINEL]) * (1 << 18) and arenas[1].read() == bytes_alone
    assert asms[0].stats()["bytes_in_use"] == 0 and asms[0].stats()["reported"] == 0
    for a in asms:
        a.close()
    for p in parsers:
        p.close()


# ---- 3. the ledger's scratch table -----------------------------------------------------------------------------------
class SlotModel(Model):
    """Model with the slot rule of rule 4: a call in which more distinct streams were live with DATA (status 0, in the
    stream map behind the call), opened or closed than the scratch table has slots cannot be accounted.  DATA on ids
    the transport never knew claims no slot."""

    def __init__(self, slots, *a, **kw):
        Model.__init__(self, *a, **kw)
        self.slots, self.inmap = slots, set(self.live)

    def call(self, events, err, slices_cap, hdr_cap):
        claims = set()
        for e in events:
            k, a, b, c, d = e[:5]
            if k == EV_STREAM_OPEN and c:
                self.inmap.add(c)
                claims.add(c)
            elif k == EV_STREAM_CLOSED and c:
                claims.add(c)
                if a == 1:
                    self.inmap.discard(c)
        claims |= {e[3] for e in events if e[0] == EV_FRAME and e[1] == 0 and (e[2] >> 8) == 0 and e[3] in self.inmap}
        if len(claims) > self.slots:
            for e in events:                          # (the stream map moved on all the same)
                if e[0] == EV_STREAM_OPEN:
                    self.live.add(e[3])
                elif e[0] == EV_STREAM_CLOSED:
                    self.live.discard(e[3])
            return self.lost_call()
        return Model.call(self, events, err, slices_cap, hdr_cap)


def _ledger(g, prefix, streams, stream_window=1 << 20, conn_window=1 << 24):
    h = FH(g, prefix=prefix, streams=streams, stream_window=stream_window, conn_window=conn_window, table_slots=SLOTS)
    h.model = SlotModel(SLOTS, stream_window, conn_window, 0, 64, streams)
    return h


def _account(h, slices):
    return h.feed(slices, ev_cap=1 << 16)


def _sources(rng, ids):
    return {s: Src(rng, [rng.choice([0, 3, 60, 500]) for _ in range(400)]) for s in ids}


def _many_small_frames(rng, src, nframes, heavy=None):
    """nframes DATA frames of 1 .. 50 bytes, the streams interleaved at random, packed twenty to a slice"""
    ids = sorted(src)
    frames, sums = [], {s: 0 for s in ids}
    for _ in range(nframes):
        s = heavy if heavy is not None and rng.randrange(3) == 0 else rng.choice(ids)
        part = src[s].take(rng.randrange(1, 51))
        assert part
        sums[s] += len(part)
        frames.append(frame(0, 0, s, part))
    return [b"".join(frames[i:i + 20]) for i in range(0, len(frames), 20)], sums


@pytest.mark.parametrize("side", ["client", "server"])
def test_ledger_concurrent_claims_on_colliding_keys(gpu, side):
    """thousands of events claim the same eight colliding keys at once, from many waves of many workgroups"""
    rng = random.Random(31 if side == "client" else 32)
    src = _sources(rng, WRAP8)
    slices, sums = _many_small_frames(rng, src, 2400)
    if side == "client":
        h = _ledger(gpu, False, WRAP8)
    else:
        h = _ledger(gpu, True, ())
        slices = [PREFACE + frame(4, 0, 0)] + [frame(1, 4, s, b"\x82\x86") for s in WRAP8] + slices
    res, wire = _account(h, slices)
    assert res[0] == 9 and res[5] == 0 and res[7] == 0 and res[3] == res[4] == sum(sums.values())
    assert sorted(h.model.frames[1:]) == sorted(sums.items()) and h.model.frames[0] == (0, res[3])
    res, _ = _account(h, _many_small_frames(rng, src, 300)[0])   # (the scratch table is cleared between calls)
    assert res[0] == 9 and res[5] == 0
    h.close()


def test_ledger_first_violator_among_colliding_keys(gpu):
    rng = random.Random(33)
    slices, sums = _many_small_frames(rng, _sources(rng, WRAP8), 2400, heavy=63)
    window = (sums[63] + max(n for s, n in sums.items() if s != 63)) // 2
    assert max(n for s, n in sums.items() if s != 63) < window < sums[63]
    h = _ledger(gpu, False, WRAP8, stream_window=window)
    res, _ = _account(h, slices)
    assert res[5] == STREAM and res[6] == 63 and h.model.stats["stream_overflows"] == 1 and res[0] == 9
    h.close()


def _open_and_reset(ids):
    out = []
    for s in ids:
        out += [frame(1, 4, s, b"\x82"), frame(0, 0, s, grpc_msg(bytes([s % 251]) * (s % 40))), frame(3, 0, s, RST)]
    return out


def test_ledger_table_full(gpu):
    """k streams opened and reset one after the other in one call: the map never holds more than one, the scratch
    table needs a slot for each"""
    ids16 = list(range(1, 33, 2))
    h = _ledger(gpu, True, ())
    res, wire = _account(h, [PREFACE + frame(4, 0, 0)] + _open_and_reset(ids16))
    assert res[0] == 1 and res[5] == 0 and res[7] == 0 and res[3] == sum(5 + s % 40 for s in ids16)   # (closed streams get no frame)
    assert h.parser.live_streams() == 0
    h.close()
    # seventeen: the call is lost
    ids17 = list(range(1, 35, 2))
    h = _ledger(gpu, True, ())
    res, wire = _account(h, [PREFACE + frame(4, 0, 0)])
    assert res[:3] == (0, 0, 0) and h.model.stats["calls"] == 1
    announced = h.model.announced
    res, wire = _account(h, _open_and_reset(ids17))    # (account: -GRDMA_ERR_CAPACITY, the result block, nothing written)
    assert res == (0, 0, 0, 0, 0, LOST, 0, 2) and wire == b""
    assert h.fc.stats()["announced"] == announced == h.model.announced and h.model.stats["calls"] == 1
    # the flag stays in the next call's result, which is otherwise exact
    res, wire = _account(h, [frame(1, 4, 35, b"\x82"), frame(0, 0, 35, grpc_msg(b"next" * 9)), frame(0, 0, 1, b"gone")])
    assert res == (2, 2, 26, 41 + 4, 41, LOST, 0, 0) and h.model.frames == [(0, 45), (35, 41)]
    assert h.fc.stats()["lost"] and h.model.stats["calls"] == 2
    h.close()


def test_ledger_unknown_ids_claim_no_slot(gpu):
    unknown = list(range(101, 181, 2))
    assert len(unknown) == 40
    h = _ledger(gpu, False, (31, 63))
    frames = [frame(0, 0, s, b"u" * (s % 7 + 1)) for s in unknown]
    frames[5:5] = [frame(0, 0, 31, grpc_msg(b"a" * 30))]
    frames[20:20] = [frame(0, 0, 63, grpc_msg(b"b" * 70)), frame(0, 0, 31, grpc_msg(b""))]
    res, wire = _account(h, frames)
    total = sum(s % 7 + 1 for s in unknown) + 35 + 75 + 5
    assert res[5] == 0 and res[7] == 0 and res[3] == total and res[4] == 115
    assert h.model.frames == [(0, total), (31, 40), (63, 75)] and not h.fc.stats()["lost"]
    h.close()
