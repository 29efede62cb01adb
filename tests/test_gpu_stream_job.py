"""GPU parity of the device-resident streaming job (what bench.py times): rounds of
{rdma_flush step, wire, endpoint-read loop until it would block} for a list of framed
gRPC messages, against the CPU oracle driving the same loop
(rdma_bp_posix.cc:470-524 rdma_flush, :180-291 rdma_do_read / rdma_continue_read).

Both schedules are covered: the sequential one (five kernels per round in stream order)
and the pipelined one (neighbouring rounds overlap on side streams).  With rounds of
at most ring/6 the pipelined schedule must reproduce the sequential slices exactly;
with a small ring the credit may arrive a round later, the records may be cut at
other places, and the delivered BYTE STREAM is what has to match -- for the stream-ordered
pipeline, whose credit visibility depends on timing.  The PAIRED graph (the default schedule,
what bench.py times) is a chain: its credit lag is exactly one round, the oracle can be driven
the same way, and the last test of this file asserts bit-exact slices, ring and state at
credit-limited rings too.
"""
import random

import pytest

from oracle import pyorc
from tests.stream_job_lib import (PASSES, _advance, _fast_counts, _run_job, _table_cache_stats, check_rx_state, framed,
                                  rx_state_of)

pytestmark = pytest.mark.gpu


def _framed_slices(n_msgs, msg_len, seed):
    """Slice list of n_msgs framed messages exactly as chttp2 hands them to the endpoint."""
    rng = random.Random(seed)
    out = []
    for i in range(n_msgs):
        msg = bytes(rng.getrandbits(8) for _ in range(64)) * (msg_len // 64) + bytes(msg_len % 64)
        wire, lens = pyorc.h2_frame_message(msg, stream_id=2 * i + 1)
        off = 0
        for n in lens:
            out.append(wire[off:off + n])
            off += n
    return out


def _oracle_passes(R, max_sge, slices, sends=1, passes=PASSES):
    """The reference loop on the CPU: one Send from the rdma_flush cursor, then endpoint
    reads until one would block; repeat until the list is gone.  `passes` times over the
    same link; returns (delivered slices, rounds, states, ring image) after every pass."""
    o = pyorc.OracleLink(R, max_sge)
    out = []
    for _ in range(passes):
        idx, byte = 0, 0
        delivered, rounds = [], 0
        while idx < len(slices):
            for _k in range(sends):  # (sends > 1: rdma_flush sends again while the write holds data, then the peer drains)
                if idx >= len(slices):
                    break
                sent = o.send(0, slices[idx:], byte)
                left = sent
                while left > 0:  # advance the cursor like rdma_flush does
                    room = len(slices[idx]) - byte
                    if left >= room:
                        left -= room
                        idx += 1
                        byte = 0
                    else:
                        byte += left
                        left = 0
            rounds += 1
            while True:
                s, _alloc = o.endpoint_read(1)
                if not s:
                    break
                delivered.append(s)
            assert rounds < 100000
        out.append((delivered, rounds, (o.state(0), rx_state_of(o)), o.ring_mem(1)))
    o.close()
    return out


def _oracle_rounds(R, max_sge, slices, sends=1):
    """PASSES passes of the reference loop; returns the slices of the last pass and the rounds of the first."""
    per_pass = _oracle_passes(R, max_sge, slices, sends)
    delivered, _rounds, st, ring = per_pass[-1]
    return delivered, per_pass[0][1], st, ring


CASES = [
    # (ring, max_sge, n_msgs, msg_len)
    (1 << 22, 4095, 6, 1 << 20),      # reference default ring, 1 MiB messages: every round is cut by the staging budget
    (1 << 24, 4095, 40, 70000),       # 16 MiB ring, many medium messages: rounds limited by max_sge / staging
    (1 << 18, 30, 24, 3000),          # small ring, reference default max_sge = 30
    (1 << 26, 512, 24, 1 << 18),      # big ring, rounds of 512 records (~6 MiB = ring/10): no Send is credit-limited
]


@pytest.mark.parametrize("case", CASES, ids=["r4m_1mib", "r16m_70k", "r256k_sge30", "r64m_sge512"])
def test_sequential_job_matches_oracle_rounds(gpu, case):
    R, max_sge, n_msgs, msg_len = case
    slices = _framed_slices(n_msgs, msg_len, seed=R % 97)
    exp, exp_rounds, (st0, st1), ring = _oracle_rounds(R, max_sge, slices)
    got = _run_job(gpu, R, max_sge, slices, pipeline=False)
    assert [len(x) for x in got["slices"]] == [len(x) for x in exp]
    assert got["slices"] == exp
    assert got["rounds"] == exp_rounds
    assert got["ring"] == ring == bytes(R)
    for k in ("remote_tail", "remote_head", "partial_write"):
        assert got["tx"][k] == st0[k], k
    check_rx_state(got["rx"], st1)


@pytest.mark.parametrize("flags", [0, 2], ids=["staged", "direct"])
@pytest.mark.parametrize("case", CASES, ids=["r4m_1mib", "r16m_70k", "r256k_sge30", "r64m_sge512"])
def test_pipelined_job_delivers_the_same_stream(gpu, case, flags):
    R, max_sge, n_msgs, msg_len = case
    slices = _framed_slices(n_msgs, msg_len, seed=R % 97)
    want = b"".join(slices)
    seq = _run_job(gpu, R, max_sge, slices, pipeline=False, flags=flags)
    pip = _run_job(gpu, R, max_sge, slices, pipeline=True, flags=flags)
    assert b"".join(seq["slices"]) == want
    assert b"".join(pip["slices"]) == want
    assert pip["ring"] == bytes(R), "ring not zero after the pipelined drain"
    assert pip["rx"]["head"] == pip["tx"]["remote_tail"]
    assert pip["rx"]["remain"] == 0
    if max_sge == 512:
        # no Send is ever limited by the credit: the pipelined schedule makes the same
        # records, hence the same endpoint reads, as the sequential one
        assert [len(x) for x in pip["slices"]] == [len(x) for x in seq["slices"]]
        assert pip["rx"] == seq["rx"] and pip["tx"]["remote_tail"] == seq["tx"]["remote_tail"]


# Streams whose record sizes are periodic and whose rounds are cut by max_sge (not by the staging budget): the
# steady state k_rx_fast (csrc/grdma_rx_fast.hip) takes.  An ODD max_sge makes every other round end behind a
# frame-header slice (the next round starts with a read of capacity 247 left open); several passes over a ring of a
# few rounds walk the ring end through the records and cross the credit threshold (ring / 2) inside a drain.
FAST_CASES = [
    # (ring, max_sge, n_msgs, msg_len)
    (1 << 24, 255, 40, 1 << 17),
    (1 << 25, 511, 36, 1 << 18),
    (1 << 23, 130, 48, 40000),
]


@pytest.mark.parametrize("flags", [0, 2], ids=["staged", "direct"])
@pytest.mark.parametrize("pipeline", [False, True], ids=["sequential", "pipelined"])
@pytest.mark.parametrize("case", FAST_CASES, ids=["r16m_sge255", "r32m_sge511", "r8m_sge130"])
def test_steady_state_drains_through_the_fast_planner_match_the_oracle(gpu, case, pipeline, flags):
    R, max_sge, n_msgs, msg_len = case
    slices = _framed_slices(n_msgs, msg_len, seed=R % 89)
    exp, exp_rounds, (st0, st1), ring = _oracle_rounds(R, max_sge, slices)
    before = _fast_counts(gpu)
    got = _run_job(gpu, R, max_sge, slices, pipeline=pipeline, flags=flags)
    after = _fast_counts(gpu)
    assert [len(x) for x in got["slices"]] == [len(x) for x in exp]
    assert got["slices"] == exp
    assert got["rounds"] == exp_rounds
    assert got["ring"] == ring == bytes(R)
    for k in ("remote_tail", "remote_head", "partial_write"):
        assert got["tx"][k] == st0[k], k
    check_rx_state(got["rx"], st1)
    took = after[0] - before[0]
    assert took >= exp_rounds, "k_rx_fast took %d drains (declined by reason: %s)" % (
        took, [a - b for a, b in zip(after[1:6], before[1:6])])
    # every Send of the three passes is priced from the index of the slice buffer (either wire, no empty slice)
    assert after[6] - before[6] >= PASSES * exp_rounds and after[7] == before[7], (after[6:], before[6:])


# Drains of more than 1024 records: the multi-workgroup drain plan of the paired schedule (csrc/grdma_rx_multi.h:
# workgroup b lays out records [1024 b, 1024 b + 1024) from closed forms over the pattern, nothing exchanged between
# the workgroups).  An odd max_sge (every other drain starts with a read left open), rings of a few rounds (the ring
# end and the credit threshold walk through the records of every workgroup), a six-record pattern with 16 KiB
# payloads and a two-record pattern of small ones; the last case has no record that closes a read (all < 512
# bytes): the body declines in every workgroup and the last one to arrive runs the general planner.
MULTI_CASES = [
    # (ring, max_sge, n_msgs, msg_len, taken by the steady-state body)
    # (rounds of at most ring / 6: no Send of the paired schedule is credit-limited, the plain oracle rounds apply)
    (1 << 23, 3001, 6000, 600, True),
    (1 << 26, 2049, 1400, 20000, True),
    (1 << 25, 4095, 8000, 1500, True),
    (1 << 22, 1500, 3000, 100, False),
]


@pytest.mark.parametrize("flags", [0, 2], ids=["staged", "direct"])
@pytest.mark.parametrize("case", MULTI_CASES, ids=["r8m_sge3001", "r64m_sge2049", "r32m_sge4095", "r4m_sge1500_small"])
def test_drains_of_several_workgroups_match_the_oracle(gpu, case, flags):
    R, max_sge, n_msgs, msg_len, taken = case
    rng = random.Random(R % 97)
    body = bytes(rng.getrandbits(8) for _ in range(msg_len))
    slices = []
    for i in range(n_msgs):
        wire, lens = pyorc.h2_frame_message(body, stream_id=2 * i + 1)
        off = 0
        for n in lens:
            slices.append(wire[off:off + n])
            off += n
    exp, exp_rounds, (st0, st1), ring = _oracle_rounds(R, max_sge, slices)
    before = _fast_counts(gpu)
    tab0 = _table_cache_stats(gpu)
    got = _run_job(gpu, R, max_sge, slices, pipeline=True, flags=flags)
    after = _fast_counts(gpu)
    tab1 = _table_cache_stats(gpu)
    assert [len(x) for x in got["slices"]] == [len(x) for x in exp]
    assert got["slices"] == exp
    assert got["ring"] == ring == bytes(R)
    for k in ("remote_tail", "remote_head", "partial_write"):
        assert got["tx"][k] == st0[k], k
    check_rx_state(got["rx"], st1)
    took = after[0] - before[0]
    if taken:
        assert took >= exp_rounds, "the steady-state bodies took %d drains (declined by reason: %s)" % (
            took, [a - b for a, b in zip(after[1:6], before[1:6])])
        # round 5: the read-state tables of a periodic stream are computed once per rotation of the pattern and kept with
        # the connection; the job runs its passes (calibration, graph) over the same stream, so most drains find them
        hits, fills = tab1[0] - tab0[0], tab1[1] - tab0[1]
        assert hits + fills >= exp_rounds and hits >= 1 and fills >= 1, (hits, fills, exp_rounds)


SENDS_CASES = [
    # (exact cases: rounds of at most ring / 6, as MULTI_CASES)
    (1 << 27, 1023, 90, 1 << 18, True),     # messages of 34 slices: rounds of two Sends of 1023 slices
    (1 << 25, 4095, 8000, 1500, True),      # two Sends of 4095 records per round: 8190 records per drain
    (1 << 24, 2500, 3000, 100, None),       # tiny messages: 9000 records, the second Send of a round ends the write
                                            # (exact; the predicting drain bodies decline them, as in MULTI_CASES)
    (1 << 22, 700, 40, 1 << 18, False),     # a ring the rounds fill: the second Send is cut by the free space
    # bench.py's headline configuration itself (`value`): 256 x 1 MiB messages of 130 slices, 256 MiB ring, max_sge
    # 4095, two Sends per round -- rounds of 63 / 63 / 63 / 63 / 4 messages; a Send is priced with the credits of the
    # drains two rounds back and three rounds (189 MiB + tags) fit the ring, so the oracle's plain rounds apply
    (1 << 28, 4095, 256, 1 << 20, True),
]


@pytest.mark.parametrize("case", [(1 << 22, 30, 64, 48, 1 << 20), (1 << 18, 30, 1, 120, 9000), (1 << 20, 64, 2, 12, 200000),
                                  (1 << 22, 700, 2, 40, 1 << 18), (1 << 23, 255, 1, 40, 1 << 17)],
                         ids=["r4m_sge30x64", "r256k_sge30", "r1m_sge64x2", "r4m_sge700x2", "r8m_sge255"])
def test_paired_schedule_with_promised_credit_equals_the_plain_oracle_rounds(gpu, case):
    """grdma_stream_job_set_promised_credit: inside the planner pair's launch the Send of round t + 1 waits for the
    drain plan of round t and is priced with the credit that drain's scatter will post.  The paired schedule then has
    no round of credit lag: at rings every round fills -- the reference's 4 MiB default with max_sge 30, 256 KiB, 1 MiB
    -- slices, ring image and state equal the oracle's PLAIN rounds (Send(s), endpoint reads until one would block),
    which the paired schedule otherwise only matches with the credit a round late."""
    R, max_sge, sends, n_msgs, msg_len = case
    rng = random.Random(R % 73 + sends)
    body = bytes(rng.getrandbits(8) for _ in range(min(msg_len, 4096))) * (msg_len // min(msg_len, 4096) + 1)
    slices = []
    for i in range(n_msgs):
        wire, lens = pyorc.h2_frame_message(body[:msg_len], stream_id=2 * i + 1)
        off = 0
        for ln in lens:
            slices.append(wire[off:off + ln])
            off += ln
    import ctypes as C
    lib = gpu.load()
    pc0 = (C.c_uint64 * 4)()
    lib.grdma_tx_promise_counts(pc0)
    got = _run_job(gpu, R, max_sge, slices, pipeline=True, flags=0, sends=sends, promise=True)
    pc1 = (C.c_uint64 * 4)()
    lib.grdma_tx_promise_counts(pc1)
    counts = [int(b) - int(a) for a, b in zip(pc0, pc1)]
    print("promised-credit Sends: priced with it %d, none in the drain %d, older block %d, waits that ran out %d" % tuple(counts))
    assert counts[3] == 0 and counts[0] > 0, counts
    exp, exp_rounds, (st0, st1), ring = _oracle_rounds(R, max_sge, slices, sends=sends)
    assert b"".join(got["slices"]) == b"".join(slices)
    assert [len(x) for x in got["slices"]] == [len(x) for x in exp]
    assert got["slices"] == exp
    assert got["ring"] == ring == bytes(R)
    for k in ("remote_tail", "remote_head", "partial_write"):
        assert got["tx"][k] == st0[k], k
    check_rx_state(got["rx"], st1)


@pytest.mark.parametrize("promise", [True, False], ids=["promised", "credit_a_round_late"])
@pytest.mark.parametrize("case", [(1 << 22, 30, 64, 24, 1 << 20), (1 << 18, 30, 1, 120, 9000), (1 << 24, 4095, 1, 40, 70000)],
                         ids=["r4m_sge30x64", "r256k_sge30", "r16m_sge4095"])
def test_the_wire_inside_the_planner_pairs_launch_delivers_what_a_wire_launch_of_its_own_delivers(gpu, case, promise):
    """Round 6: a paired job of few links with small rings carries the wire of a round in the launch of the planner pair
    -- wire workgroups in front of the drain's, which wait for them before they look at the ring -- instead of a k_copy
    launch of its own (grdma_stream_job_set_fused_wire; two launches per round).  Same job with the fused wire and
    without: the graph has no wire launches in the first case and one per round in the second, no drain's wait ran out,
    and slices, ring image and state of both are the oracle's (plain rounds with the promised credit; without it the
    two runs must agree with each other and deliver the stream)."""
    R, max_sge, sends, n_msgs, msg_len = case
    slices = _framed_slices(n_msgs, msg_len, seed=R % 89 + sends)
    lib = gpu.load()
    ran_out0 = int(lib.grdma_wire_wait_runouts())
    runs = {}
    for fw in (True, False):
        runs[fw] = _run_job(gpu, R, max_sge, slices, pipeline=True, flags=0, sends=sends, promise=promise, fused_wire=fw)
    assert int(lib.grdma_wire_wait_runouts()) == ran_out0
    on, off = runs[True], runs[False]
    assert on["wire_groups"] >= 8 and off["wire_groups"] == 0, (on["wire_groups"], off["wire_groups"])
    # (launches by class in the last, instrumented-or-graph pass: class 2 is the wire)
    print("launches by class: fused %s, separate %s" % (on["launches"], off["launches"]))
    assert b"".join(on["slices"]) == b"".join(slices)
    for k in ("slices", "ring", "tx", "rx"):
        assert on[k] == off[k], k
    if promise:
        exp, _rounds, (st0, st1), ring = _oracle_rounds(R, max_sge, slices, sends=sends)
        assert on["slices"] == exp
        assert on["ring"] == ring == bytes(R)
        for k in ("remote_tail", "remote_head", "partial_write"):
            assert on["tx"][k] == st0[k], k
        check_rx_state(on["rx"], st1)


@pytest.mark.parametrize("case", [(1 << 20, 30, 64, 40, 200000), (1 << 22, 30, 64, 14, 1 << 20)], ids=["r1m_sge30x64", "r4m_sge30x64"])
def test_promised_credit_with_mixed_message_sizes_equals_the_plain_oracle_rounds(gpu, case):
    """The reference's own test distribution -- message sizes uniform in [1, max] (examples/cpp/test/common.h:4-31) -- at
    its default max_sge of 30, rounds of up to 64 Sends, paired schedule with the promised credit and (on one link with
    a small ring) the wire inside the planner pair's launch: what bench.py times as value_mixed_sizes_ring4096_sge30.
    No period in the record sizes: the drains are predicted from the sizes their own Sends computed (rxh_body) and
    verified in the ring.  Slices, ring image and state equal the oracle's plain rounds."""
    R, max_sge, sends, n_msgs, max_len = case
    rng = random.Random(R % 71 + n_msgs)
    slices = []
    for i in range(n_msgs):
        ln = rng.randrange(1, max_len)
        body = bytes(rng.getrandbits(8) for _ in range(min(ln, 2048))) * (ln // min(ln, 2048) + 1)
        wire, lens = pyorc.h2_frame_message(body[:ln], stream_id=2 * i + 1)
        off = 0
        for l in lens:
            slices.append(wire[off:off + l])
            off += l
    got = _run_job(gpu, R, max_sge, slices, pipeline=True, flags=0, sends=sends, promise=True)
    assert got["wire_groups"] > 0
    exp, _rounds, (st0, st1), ring = _oracle_rounds(R, max_sge, slices, sends=sends)
    assert b"".join(got["slices"]) == b"".join(slices)
    assert [len(x) for x in got["slices"]] == [len(x) for x in exp]
    assert got["slices"] == exp
    assert got["ring"] == ring == bytes(R)
    for k in ("remote_tail", "remote_head", "partial_write"):
        assert got["tx"][k] == st0[k], k
    check_rx_state(got["rx"], st1)


def test_three_links_of_one_job_with_two_sends_per_round_and_promised_credit(gpu):
    """Three connections with different rings and max_sge in ONE job (one op per connection in every launch), two Sends
    per round and the promised credit: every link's slices, ring image and state equal the oracle's plain rounds of that
    link -- the planner workgroups of a launch are indexed by link, the hand-over of a link's drain plan to its Send is
    per link."""
    from grpc_rdma_amd import stream as gs
    global PASSES
    cfgs = [(1 << 20, 64, 12, 200000), (1 << 19, 30, 20, 70000), (1 << 21, 100, 9, 300000)]
    links, keep, all_slices = [], [], []
    for li, (R, max_sge, n_msgs, msg_len) in enumerate(cfgs):
        rng = random.Random(100 + li)
        body = bytes(rng.getrandbits(8) for _ in range(4096)) * (msg_len // 4096 + 1)
        slices = []
        for i in range(n_msgs):
            wire, lens = pyorc.h2_frame_message(body[:msg_len], stream_id=2 * i + 1)
            off = 0
            for ln in lens:
                slices.append(wire[off:off + ln])
                off += ln
        bufs = [gpu.DeviceBuffer(data=s, offset=rng.randrange(16)) for s in slices]
        tx, rx = gpu.Pair(R, max_sge, 0), gpu.Pair(R, max_sge, 0)
        gpu.connect_pairs(tx, rx)
        N = sum(len(s) for s in slices)
        dst_cap = N + 32 * (2 * len(slices) + 64) + 4096
        dst = gpu.DeviceBuffer(nbytes=dst_cap)
        links.append((tx, rx, [(b.ptr, len(s)) for b, s in zip(bufs, slices)], dst.ptr, dst_cap, 2 * len(slices) + 64))
        keep.append((tx, rx, dst, dst_cap, bufs, R, max_sge, N))
        all_slices.append(slices)
    job = gs.MultiStreamJob(links, 60)
    job.set_pipeline(True)
    job.set_sends(2)
    job.set_promised_credit(True)
    total = sum(k[7] for k in keep)
    for p in range(PASSES):
        r = job.run(gs.RUN_EAGER if p == 0 else gs.RUN_GRAPH)
        assert r.done and r.bytes_delivered == total
        if p == 0:
            job.set_rounds(30)
    for li, (tx, rx, dst, dst_cap, _bufs, R, max_sge, _n) in enumerate(keep):
        exp, _rounds, (st0, st1), ring = _oracle_rounds(R, max_sge, all_slices[li], sends=2)
        mem = dst.read(dst_cap)
        got = [mem[o:o + n] for o, n in job.delivered_slices(li)]
        assert got == exp, "link %d" % li
        assert rx.ring_mem() == ring == bytes(R)
        for k in ("remote_tail", "remote_head", "partial_write"):
            assert tx.state()[k] == st0[k], (li, k)
        check_rx_state(rx.state(), st1, li)
    job.close()
    for tx, rx, *_ in keep:
        tx.close()
        rx.close()


FOLDED_CASES = [
    # (ring, max_sge, sends, n_msgs, msg_len, exact): more than two Sends per round -- priced as ONE cut of the index
    (1 << 25, 30, 8, 40, 1 << 18, True),      # the reference's max_sge: rounds of eight Sends of 30 slices
    (1 << 26, 100, 6, 30, 1 << 20, True),     # 1 MiB messages, 600 slices per round
    (1 << 24, 7, 64, 2000, 300, None),        # tiny messages, 64 Sends of 7 slices (the drain bodies decline them)
    (1 << 22, 30, 64, 48, 1 << 20, False),    # the reference's default knobs: every round is cut by the free space
    (1 << 18, 30, 16, 30, 50000, "declines"), # a 256 KiB ring: a Send of 30 slices exceeds the staging budget (ring / 2):
                                              # the folded pricing declines, the general planner sends one Send per round
]


@pytest.mark.parametrize("pipeline", [True, False], ids=["paired", "sequential"])
@pytest.mark.parametrize("flags", [0, 2], ids=["staged", "direct"])
@pytest.mark.parametrize("case", FOLDED_CASES, ids=["r32m_sge30x8", "r64m_sge100x6", "r16m_sge7x64", "r4m_sge30x64", "r256k_sge30x16"])
def test_many_sends_per_round_priced_as_one_cut_of_the_index_match_the_oracle(gpu, case, flags, pipeline):
    """grdma_stream_job_set_sends(n > 2): the Sends of a round folded into one pricing (csrc/grdma_tx_multi.h: every Send
    but the last takes max_sge whole records, the staging budget of one Send binds nowhere, so the round is one cut of
    the index against the free space; tx_rounds, the last Send's result and partial_write_ in closed form).  Slices,
    ring image and state equal the oracle's rounds of n Sends and one drain; where every round is cut by the ring's
    free space the paired schedule sees its credit a round late and the byte stream + the empty ring are checked --
    the SEQUENTIAL schedule (five launches per round, the same planner workgroups) sees it at once and equals the
    oracle's rounds there too (the reference's default knobs: 4 MiB ring, max_sge 30)."""
    R, max_sge, sends, n_msgs, msg_len, exact = case
    if not pipeline and exact is False:
        exact = True
    rng = random.Random(R % 79 + sends)
    body = bytes(rng.getrandbits(8) for _ in range(min(msg_len, 4096))) * (msg_len // min(msg_len, 4096) + 1)
    slices = []
    for i in range(n_msgs):
        wire, lens = pyorc.h2_frame_message(body[:msg_len], stream_id=2 * i + 1)
        off = 0
        for ln in lens:
            slices.append(wire[off:off + ln])
            off += ln
    before = _fast_counts(gpu)
    got = _run_job(gpu, R, max_sge, slices, pipeline=pipeline, flags=flags, sends=sends)
    after = _fast_counts(gpu)
    assert b"".join(got["slices"]) == b"".join(slices)
    assert got["ring"] == bytes(R)
    if exact != "declines":
        assert after[6] - before[6] > 0 and after[7] == before[7], "Sends priced from the index / declined: %d / %d" % (
            after[6] - before[6], after[7] - before[7])
    else:
        assert after[7] > before[7]
    if exact in (True, None):
        exp, exp_rounds, (st0, st1), ring = _oracle_rounds(R, max_sge, slices, sends=sends)
        assert [len(x) for x in got["slices"]] == [len(x) for x in exp]
        assert got["slices"] == exp
        for k in ("remote_tail", "remote_head", "partial_write"):
            assert got["tx"][k] == st0[k], k
        check_rx_state(got["rx"], st1)


@pytest.mark.parametrize("flags", [0, 2], ids=["staged", "direct"])
@pytest.mark.parametrize("case", SENDS_CASES, ids=["r128m_sge1023", "r32m_sge4095", "r16m_small", "r4m_ring_limited", "r256m_headline"])
def test_two_sends_per_round_in_one_plan_match_the_oracle(gpu, case, flags):
    """grdma_stream_job_set_sends(2): a round's plan holds two consecutive Sends (rdma_flush's loop while the ring has
    room), priced one after the other from the index by the small planner workgroups (csrc/grdma_tx_multi.h), their
    records back to back in gather plan, staging buffer and ring; the drain of the round lays out both Sends' records
    (32 workgroups).  Slices, ring image and state equal the oracle driven the same way: Send, Send, endpoint reads
    until one would block.  (The ring-limited case: the paired schedule sees the credit a round late -- the byte
    stream and the empty ring are checked, the oracle's rounds are not the job's.)"""
    R, max_sge, n_msgs, msg_len, exact = case
    rng = random.Random(R % 83)
    body = bytes(rng.getrandbits(8) for _ in range(min(msg_len, 4096))) * (msg_len // min(msg_len, 4096) + 1)
    slices = []
    for i in range(n_msgs):
        wire, lens = pyorc.h2_frame_message(body[:msg_len], stream_id=2 * i + 1)
        off = 0
        for ln in lens:
            slices.append(wire[off:off + ln])
            off += ln
    before = _fast_counts(gpu)
    got = _run_job(gpu, R, max_sge, slices, pipeline=True, flags=flags, sends=2)
    after = _fast_counts(gpu)
    assert b"".join(got["slices"]) == b"".join(slices)
    assert got["ring"] == bytes(R)
    if exact is not False:
        exp, exp_rounds, (st0, st1), ring = _oracle_rounds(R, max_sge, slices, sends=2)
        assert [len(x) for x in got["slices"]] == [len(x) for x in exp]
        assert got["slices"] == exp
        for k in ("remote_tail", "remote_head", "partial_write"):
            assert got["tx"][k] == st0[k], k
        check_rx_state(got["rx"], st1)
        if exact is True:
            assert after[0] - before[0] >= exp_rounds, "drains taken by the predicting bodies: %d of %d rounds per pass" % (
                after[0] - before[0], exp_rounds)


@pytest.mark.parametrize("flags", [0, 2], ids=["staged", "direct"])
@pytest.mark.parametrize("case", FAST_CASES[:2], ids=["r16m_sge255", "r32m_sge511"])
def test_the_instrumented_schedule_is_the_graphs_chain(gpu, case, flags):
    """GRDMA_RUN_INSTRUMENTED_SCHEDULE (bench.py's roofline of the fused scatter + gather launch): the launches of
    the paired schedule one by one with events between them -- the same slices, ring and state as the oracle's
    rounds, one planner pair per round, one fused launch per round but the last."""
    from grpc_rdma_amd import stream as gs
    R, max_sge, n_msgs, msg_len = case
    slices = _framed_slices(n_msgs, msg_len, seed=R % 89)
    exp, exp_rounds, (st0, st1), ring = _oracle_rounds(R, max_sge, slices)
    got = _run_job(gpu, R, max_sge, slices, pipeline=True, flags=flags, mode=gs.RUN_INSTRUMENTED_SCHEDULE)
    assert got["slices"] == exp
    assert got["ring"] == ring == bytes(R)
    for k in ("remote_tail", "remote_head", "partial_write"):
        assert got["tx"][k] == st0[k], k
    check_rx_state(got["rx"], st1)
    n = got["rounds_set"]
    la = dict(zip(gs.CLASS_NAMES, got["launches"]))
    assert la["plan_pair"] == n and la["scatter_gather"] == n - 1 and la["rx_apply"] == 1, la
    # (a direct wire has no wire kernel; a job of few links with rings of at most 16 MiB carries the wire in the planner
    #  pair's launch -- grdma_stream_job_wire_groups)
    assert (got["wire_groups"] > 0) == (flags == 0 and R <= (16 << 20)), got["wire_groups"]
    assert la["tx_plan"] == 1 and la["gather"] == 1 and la["wire"] == (0 if (flags & 2 or got["wire_groups"]) else n), la
    assert la["rx_plan"] == 0
    assert all(m >= 0 for m in got["ms"])


_ORACLE_FIVE_PASSES = []  # (the reference of the next test: computed once, shared by its four cases, never changed)


@pytest.mark.parametrize("flags", [0, 2], ids=["staged", "direct"])
@pytest.mark.parametrize("pipeline", [False, True], ids=["sequential", "pipelined"])
def test_the_in_order_timed_pass_and_the_stream_launch_match_the_oracle(gpu, pipeline, flags):
    """GRDMA_RUN_INSTRUMENTED (the five launches of every round in order, an event behind each) and
    grdma_stream_job_launch_streams (the sequential chain, or the limit-driven schedule over four streams for a pipelined
    job) behind the usual three passes, at the small ring with the reference's max_sge: slices, ring image and state
    equal the oracle's rounds after each of the two passes.  The timed pass counts one launch per round in every class
    -- none in `wire` on a direct wire, where the gather writes the peer ring."""
    from grpc_rdma_amd import stream as gs
    R, max_sge, n_msgs, msg_len = CASES[2]
    slices = _framed_slices(n_msgs, msg_len, seed=R % 97)
    if not _ORACLE_FIVE_PASSES:
        _ORACLE_FIVE_PASSES.extend(_oracle_passes(R, max_sge, slices, passes=PASSES + 2))
    got = _run_job(gpu, R, max_sge, slices, pipeline=pipeline, flags=flags, more_passes=(gs.RUN_INSTRUMENTED, "streams"))
    for state, (exp, _rounds, (st0, st1), ring) in zip([got] + got["more"], _ORACLE_FIVE_PASSES[PASSES - 1:]):
        assert state["slices"] == exp
        assert state["ring"] == ring == bytes(R)
        for k in ("remote_tail", "remote_head", "partial_write"):
            assert state["tx"][k] == st0[k], k
        check_rx_state(state["rx"], st1)
    assert len(got["more"]) == 2
    timed = got["more"][0]
    la = dict(zip(gs.CLASS_NAMES, timed["launches"]))
    n = got["rounds_set"]
    assert la == {"tx_plan": n, "gather": n, "wire": 0 if flags & 2 else n, "rx_plan": n, "rx_apply": n, "plan_pair": 0,
                  "scatter_gather": 0}, la
    assert all(m >= 0 for m in timed["ms"])


def test_the_instrumented_schedule_refuses_a_job_on_another_schedule(gpu):
    from grpc_rdma_amd import stream as gs
    R, max_sge, n_msgs, msg_len = FAST_CASES[0]
    slices = _framed_slices(n_msgs, msg_len, seed=3)
    with pytest.raises(Exception, match="paired schedule"):
        _run_job(gpu, R, max_sge, slices, pipeline=False, mode=gs.RUN_INSTRUMENTED_SCHEDULE)


# ---- the paired schedule at a CREDIT-LIMITED ring: exact parity with the oracle, the credit one round late --------
# The graph of a paired job is a chain: [P0] G0 W0 [X0 + P1] [A0 + G1] W1 [X1 + P2] ...  The credit of drain t is posted
# by the last workgroup of its scatter (A_t), and the send plan of round k runs in the launch in front of A_{k-1}: Send k
# sees the credits of the drains <= k - 2 of its pass (and everything of earlier passes).  That is deterministic, so the
# oracle can be driven the same way -- the sender's view of the reader's head (status_recv.remote_head) held back by one
# round -- and the job must then produce the oracle's records, slices, ring image and state EXACTLY, also where every
# Send is cut by the credit.
def _oracle_sequential_then_paired(R, max_sge, slices, paired_rounds):
    o = pyorc.OracleLink(R, max_sge)

    def drain(out):
        n = 0
        while True:
            s, _alloc = o.endpoint_read(1)
            if not s:
                return n
            out.append(s)
            n += 1

    # pass 1: the sequential rounds (every Send sees every credit)
    idx, byte, rounds = 0, 0, 0
    first = []
    while idx < len(slices):
        idx, byte = _advance(slices, idx, byte, o.send(0, slices[idx:], byte))
        rounds += 1
        drain(first)
        assert rounds < 100000
    # pass 2: the paired chain
    sender = o.p[0]
    latest = sender.status_recv.remote_head  # what the reader has reported so far
    views = []                               # views[t] = the report as it stands after drain t of this pass
    start = latest
    idx, byte = 0, 0
    delivered = []
    used = 0
    for k in range(paired_rounds):
        if idx >= len(slices):
            break
        lagged = start if k < 2 else views[k - 2]
        sender.status_recv.remote_head = lagged
        idx, byte = _advance(slices, idx, byte, o.send(0, slices[idx:], byte))
        used = k + 1
        drain(delivered)
        if sender.status_recv.remote_head != lagged:  # this drain returned credit
            latest = sender.status_recv.remote_head
        views.append(latest)
    assert idx == len(slices), "the rounds given to the paired pass do not carry the whole list"
    sender.status_recv.remote_head = latest  # (what the sender sees once the pass is over)
    st = (o.state(0), rx_state_of(o))
    ring = o.ring_mem(1)
    o.close()
    return first, rounds, delivered, used, st, ring


@pytest.mark.parametrize("flags", [0, 2], ids=["staged", "direct"])
@pytest.mark.parametrize("case", [CASES[0], (1 << 18, 30, 120, 9000), (1 << 20, 64, 12, 200000)],
                         ids=["r4m_1mib", "r256k_sge30_9k", "r1m_sge64_200k"])
def test_paired_schedule_at_a_credit_limited_ring_equals_the_oracle_with_the_credit_one_round_late(gpu, case, flags):
    from grpc_rdma_amd import stream as gs
    R, max_sge, n_msgs, msg_len = case
    slices = _framed_slices(n_msgs, msg_len, seed=R % 83)
    g = gpu
    rng = random.Random(5)
    bufs = [g.DeviceBuffer(data=s, offset=rng.randrange(16)) for s in slices]
    tx, rx = g.Pair(R, max_sge, flags), g.Pair(R, max_sge, flags)
    g.connect_pairs(tx, rx)
    N = sum(len(s) for s in slices)
    dst_cap = N + 32 * (2 * len(slices) + 64) + 4096
    dst = g.DeviceBuffer(nbytes=dst_cap)
    sge = [(b.ptr, len(s)) for b, s in zip(bufs, slices)]
    job = gs.MultiStreamJob([(tx, rx, sge, dst.ptr, dst_cap, 2 * len(slices) + 64)], 4096)
    job.set_pipeline(False)
    r = job.run(gs.RUN_EAGER)            # pass 1: sequential rounds
    assert r.done and r.bytes_delivered == N
    rounds1 = int(max(r.tx_rounds, r.rx_rounds))
    paired_rounds = 2 * rounds1 + 6      # (a Send that finds the credit of the round before not yet there sends less)
    exp1, exp_rounds1, exp2, used, (st0, st1), ring = _oracle_sequential_then_paired(R, max_sge, slices, paired_rounds)
    assert rounds1 == exp_rounds1
    mem = dst.read(dst_cap)
    assert [mem[o:o + n] for o, n in job.delivered_slices(0)] == exp1
    job.set_pipeline(True)
    job.set_rounds(paired_rounds)
    r = job.run(gs.RUN_GRAPH)            # pass 2: the paired chain
    assert r.done and r.bytes_delivered == N and r.bytes_sent == N
    print("rounds: sequential %d, paired %d of %d" % (rounds1, used, paired_rounds))
    assert used > rounds1, "this case was meant to be credit-limited in the paired pass"
    mem = dst.read(dst_cap)
    got = [mem[o:o + n] for o, n in job.delivered_slices(0)]
    assert [len(x) for x in got] == [len(x) for x in exp2]
    assert got == exp2
    assert rx.ring_mem() == ring == bytes(R)
    txs, rxs = tx.state(), rx.state()
    for k in ("remote_tail", "remote_head", "partial_write"):
        assert txs[k] == st0[k], k
    check_rx_state(rxs, st1)
    job.close()
    tx.close()
    rx.close()


# ---- both directions of ONE connection in flight (BASELINE configs[3] is bidirectional streaming; the reference's
# pair is full duplex: Recv shares nothing with Send but the queue pair, pair.cc:264-286, pair.h:171-175) -----------
@pytest.mark.parametrize("flags", [0, 2], ids=["staged", "direct"])
@pytest.mark.parametrize("pipeline", [False, True], ids=["sequential", "paired"])
def test_bidirectional_job_both_directions_of_one_pair_in_the_same_launches(gpu, pipeline, flags):
    """One pair of connected ends, TWO links of one job: a -> b and b -> a.  Every launch of the job carries both
    directions (grid.y = 2: the Send of a and the Send of b priced side by side, both rings drained by one pass, the
    credit of each direction returned through the other end's status word), so each end is sender and receiver at the
    same time.  Each direction must deliver exactly what the oracle's rounds deliver for it, ring image and state
    included -- the two directions share no protocol state."""
    from grpc_rdma_amd import stream as gs
    g = gpu
    R, max_sge = 1 << 24, 255
    fwd = _framed_slices(40, 1 << 17, seed=11)   # a -> b: 40 x 128 KiB
    bwd = _framed_slices(70, 40000, seed=12)     # b -> a: 70 x 40 kB (another number of rounds, other record sizes)
    # the oracle: one link object has both directions; a job's round = one Send per direction, then both drains
    o = pyorc.OracleLink(R, max_sge)
    exp = [[], []]
    rounds = [0, 0]
    for _ in range(PASSES):
        cur = [[0, 0], [0, 0]]
        delivered = [[], []]
        lists = [fwd, bwd]
        while cur[0][0] < len(fwd) or cur[1][0] < len(bwd):
            for d in (0, 1):
                idx, byte = cur[d]
                if idx < len(lists[d]):
                    sent = o.send(d, lists[d][idx:], byte)
                    cur[d] = list(_advance(lists[d], idx, byte, sent))
            for d in (0, 1):  # direction d is read by side 1 - d
                while True:
                    s, _alloc = o.endpoint_read(1 - d)
                    if not s:
                        break
                    delivered[d].append(s)
        exp = delivered
    st = (rx_state_of(o, 0), rx_state_of(o, 1))
    rings = (o.ring_mem(0), o.ring_mem(1))
    o.close()

    rng = random.Random(5)
    a, b = g.Pair(R, max_sge, flags), g.Pair(R, max_sge, flags)
    g.connect_pairs(a, b)
    links, keep = [], []
    for tx, rx, sl in ((a, b, fwd), (b, a, bwd)):
        bufs = [g.DeviceBuffer(data=s, offset=rng.randrange(16)) for s in sl]
        N = sum(len(s) for s in sl)
        cap = N + 32 * (2 * len(sl) + 64) + 4096
        dst = g.DeviceBuffer(nbytes=cap)
        keep.append((bufs, dst, cap, N))
        links.append((tx, rx, [(bf.ptr, len(s)) for bf, s in zip(bufs, sl)], dst.ptr, cap, 2 * len(sl) + 64))
    job = gs.MultiStreamJob(links, 6 * (keep[0][3] // (R // 2) + len(fwd) // max_sge + len(bwd) // max_sge) + 24)
    job.set_pipeline(pipeline)
    r = job.run(gs.RUN_EAGER)
    total = keep[0][3] + keep[1][3]
    assert r.done and r.bytes_delivered == total and r.bytes_sent == total
    nrounds = int(max(r.tx_rounds, r.rx_rounds))
    job.set_rounds(2 * nrounds + 4 if pipeline else nrounds + 2)
    for _ in range(PASSES - 1):
        r = job.run(gs.RUN_GRAPH)
        assert r.done and r.bytes_delivered == total
    for d in (0, 1):
        _bufs, dst, cap, _n = keep[d]
        mem = dst.read(cap)
        got = [mem[o_:o_ + n] for o_, n in job.delivered_slices(d)]
        assert [len(x) for x in got] == [len(x) for x in exp[d]], "direction %d" % d
        assert got == exp[d], "direction %d" % d
    assert a.ring_mem() == rings[0] == bytes(R) and b.ring_mem() == rings[1] == bytes(R)
    for pair_, s_ in ((a, st[0]), (b, st[1])):
        ps = pair_.state()
        for k in ("remote_tail", "remote_head", "partial_write"):
            assert ps[k] == s_[k], k
        check_rx_state(ps, s_)
    job.close()
    a.close()
    b.close()


# ---- record sizes WITHOUT a period (the reference's own test distribution: message sizes uniform in [1, max],
# examples/cpp/test/common.h:4-31): the drain of a round is predicted from the sizes its Send computed
# (csrc/grdma_rx_hint.h), verified record by record in the ring, laid out by sixteen small workgroups ---------------
@pytest.mark.parametrize("flags", [0, 2], ids=["staged", "direct"])
@pytest.mark.parametrize("case", [(1 << 25, 1023, 50, 300000, 7, 1), (1 << 24, 640, 300, 9000, 8, 1), (1 << 26, 4095, 40, 1 << 20, 9, 1),
                                  (1 << 28, 4095, 64, 2 << 20, 10, 2), (1 << 26, 2500, 6000, 900, 11, 2)],
                         ids=["r32m_sge1023", "r16m_sge640_small", "r64m_sge4095", "r256m_sge4095x2", "r64m_sge2500x2_small"])
def test_drains_without_a_period_are_predicted_from_the_sends_sizes(gpu, case, flags):
    """(x2, round 6: rounds of TWO Sends -- up to 8190 records -- the size table holds two Sends' worth and the drain loads
    its second half when the round has more than 4096 records: what bench.py's value_mixed_sizes runs)"""
    R, max_sge, n_msgs, max_len, seed, sends = case
    rng = random.Random(seed)
    slices = []
    for i in range(n_msgs):
        n = rng.randrange(1, max_len + 1)
        msg = bytes(rng.getrandbits(8) for _ in range(97)) * (n // 97) + bytes(n % 97)
        wire, lens = pyorc.h2_frame_message(msg, stream_id=2 * i + 1)
        off = 0
        for ln in lens:
            slices.append(wire[off:off + ln])
            off += ln
    exp, exp_rounds, (st0, st1), ring = _oracle_rounds(R, max_sge, slices, sends=sends)
    before = _fast_counts(gpu)
    got = _run_job(gpu, R, max_sge, slices, pipeline=True, flags=flags, sends=sends)
    after = _fast_counts(gpu)
    assert [len(x) for x in got["slices"]] == [len(x) for x in exp]
    assert got["slices"] == exp
    assert got["ring"] == ring == bytes(R)
    for k in ("remote_tail", "remote_head", "partial_write"):
        assert got["tx"][k] == st0[k], k
    check_rx_state(got["rx"], st1)
    took = after[0] - before[0]
    print("rounds %d, drains taken by a predicting body %d, declined by reason %s" % (exp_rounds, took, [a - b for a, b in zip(after[1:6], before[1:6])]))
    # (the eager first pass runs the sequential kernels, whose steady-state body needs a period: the graph passes count)
    # (a round of more than 4096 records on a connection without a period is left to the general planner whenever its
    #  period search is due -- five times in a row at first, then ever more rarely: csrc/grdma_rx_hint.h, search_due)
    searches = 5 if sends > 1 else 0
    assert took >= max(1, (PASSES - 1) * exp_rounds - 2 - searches), "drains taken by a predicting body: %d (declined by reason: %s)" % (
        took, [a - b for a, b in zip(after[1:6], before[1:6])])


# ---- round 6: the cases the round-5 review found untested ------------------------------------------------------------
def _verdict_counts(g):
    import ctypes as C
    lib = g.load()
    out = (C.c_uint64 * 2)()
    assert lib.grdma_rx_verdict_counts(out) == 0
    return [int(x) for x in out]


@pytest.mark.parametrize("flags", [0, 2], ids=["staged", "direct"])
@pytest.mark.parametrize("case", [(1 << 23, 3001, 6000, 600, 597, 3001 + 700), (1 << 25, 4095, 8000, 1500, 1497, 4095 + 750)],
                         ids=["r8m_sge3001", "r32m_sge4095"])
def test_one_drain_workgroup_declines_while_its_neighbours_accept(gpu, case, flags):
    """A periodic stream in which exactly ONE record, in the middle of a drain, carries another payload length inside the
    same encoded size (600 -> 597 bytes: both 16 + 600 on the ring; pair.cc:264-301, ring_buffer.h:180-183): every record
    behind it stays where the pattern says, the record-size history stays periodic, and the probe of ONE workgroup of
    the multi-workgroup drain plan (csrc/grdma_rx_multi.h) fails while its neighbours' pass -- they have written their
    plan entries by then.  The last workgroup to arrive runs the general planner over the same plan slots in the same
    launch (the neighbours' entries are stored write-through and acknowledged before they count in, so
    nothing of theirs is written back over the rewritten plan).  Slices, ring image and state against the oracle, and
    the verdict counter shows the mixed decline once per pass."""
    R, max_sge, n_msgs, msg_len, odd_len, odd_msg = case
    rng = random.Random(R % 97)
    body = bytes(rng.getrandbits(8) for _ in range(msg_len))
    slices = []
    for i in range(n_msgs):
        wire, lens = pyorc.h2_frame_message(body if i != odd_msg else body[:odd_len], stream_id=2 * i + 1)
        off = 0
        for n in lens:
            slices.append(wire[off:off + n])
            off += n
    # (the odd record is record 2 * odd_msg + 1 of the stream: in the middle of the third drain, a few workgroups in --
    #  not among the first records of a drain, which every workgroup reads as the pattern)
    assert len(slices) == 2 * n_msgs and len(slices[2 * odd_msg + 1]) == odd_len
    assert 256 < (2 * odd_msg + 1) % max_sge < max_sge - 256
    exp, exp_rounds, (st0, st1), ring = _oracle_rounds(R, max_sge, slices)
    before, v0 = _fast_counts(gpu), _verdict_counts(gpu)
    got = _run_job(gpu, R, max_sge, slices, pipeline=True, flags=flags)
    after, v1 = _fast_counts(gpu), _verdict_counts(gpu)
    assert [len(x) for x in got["slices"]] == [len(x) for x in exp]
    assert got["slices"] == exp
    assert got["ring"] == ring == bytes(R)
    for k in ("remote_tail", "remote_head", "partial_write"):
        assert got["tx"][k] == st0[k], k
    check_rx_state(got["rx"], st1)
    mixed, unanimous = v1[0] - v0[0], v1[1] - v0[1]
    took = after[0] - before[0]
    print("drains: %d taken by the predicting bodies, %d mixed verdicts, %d unanimous declines; declines by reason %s" % (
        took, mixed, unanimous, [a - b for a, b in zip(after[1:6], before[1:6])]))
    # the graph passes (PASSES - 1 of them; the eager first pass of a pipelined job runs the stream pipeline, whose
    # planner pair is the same kernel) each meet the odd record in one drain
    assert mixed >= PASSES - 1, (mixed, unanimous)
    assert after[3] - before[3] >= mixed      # counted as "the ring does not hold the predicted records"
    assert took >= exp_rounds                 # ... and every other drain was taken


class _LaggedLink:
    """The oracle's link driven the way the PAIRED graph runs a job (see above: Send k of a pass is priced with the
    credits of the drains <= k - 2 of that pass and everything before the pass), for either direction of the link, any
    number of passes; sequential passes (every Send sees every credit) in between.  `sends` Sends per round are priced
    from ONE view of the credit (one plan, no credit arrives inside it)."""

    def __init__(self, R, max_sge):
        self.o = pyorc.OracleLink(R, max_sge)

    def _drain(self, d, out):
        while True:
            s, _alloc = self.o.endpoint_read(1 - d)
            if not s:
                return
            out.append(s)

    def sequential_pass(self, d, slices, sends=1):
        idx, byte, rounds, out = 0, 0, 0, []
        while idx < len(slices):
            for _ in range(sends):
                if idx < len(slices):
                    idx, byte = _advance(slices, idx, byte, self.o.send(d, slices[idx:], byte))
            rounds += 1
            self._drain(d, out)
            assert rounds < 100000
        return out, rounds

    def paired_pass(self, d, slices, rounds, sends=1):
        sender = self.o.p[d]
        latest = start = sender.status_recv.remote_head
        views, out, idx, byte, used = [], [], 0, 0, 0
        for k in range(rounds):
            if idx >= len(slices):
                break
            lagged = start if k < 2 else views[k - 2]
            sender.status_recv.remote_head = lagged
            for _ in range(sends):
                if idx < len(slices):
                    idx, byte = _advance(slices, idx, byte, self.o.send(d, slices[idx:], byte))
            used = k + 1
            self._drain(d, out)
            if sender.status_recv.remote_head != lagged:
                latest = sender.status_recv.remote_head
            views.append(latest)
        assert idx == len(slices), "the rounds given to the paired pass do not carry the whole list"
        sender.status_recv.remote_head = latest
        return out, used


def _promise_counts(g):
    import ctypes as C
    lib = g.load()
    pc = (C.c_uint64 * 4)()
    lib.grdma_tx_promise_counts(pc)
    return [int(x) for x in pc]


@pytest.mark.parametrize("case", [(1 << 18, 30, 1, 120, 9000), (1 << 20, 64, 2, 12, 200000)], ids=["r256k_sge30", "r1m_sge64x2"])
def test_a_promised_credit_wait_that_runs_out_gives_the_promise_up_for_the_whole_send(gpu, case):
    """The bounded wait of the promised credit (k_plan_pair_mw: the Send workgroups of a launch wait for the drain plan
    of the same launch) made to run out in EVERY OTHER Send workgroup (grdma_debug_set_promise_wait(1): their wait is
    over before the first look).  Before round 6 such a workgroup priced with the credit posted so far while its
    neighbours priced with the promise -- one Send cut at two places.  Now the first wait to run out moves the hand-over
    word 0 -> 2 and every workgroup of the Send, whenever it looks, prices WITHOUT the promise: the launch is a launch
    of the plain paired schedule.  Checked bit for bit: when every launch of the graph passes gave the promise up the
    job's slices, ring and state are the oracle's driven with the credit one round late (the paired chain's rule); when
    none did (the emulator runs the drain's workgroups first: the promise is always kept by the time a Send looks) they
    are the oracle's plain rounds."""
    from grpc_rdma_amd import stream as gs
    import ctypes as C
    import os
    g = gpu
    R, max_sge, sends, n_msgs, msg_len = case
    rng = random.Random(R % 73 + sends)
    body = bytes(rng.getrandbits(8) for _ in range(min(msg_len, 4096))) * (msg_len // min(msg_len, 4096) + 1)
    slices = []
    for i in range(n_msgs):
        wire, lens = pyorc.h2_frame_message(body[:msg_len], stream_id=2 * i + 1)
        off = 0
        for ln in lens:
            slices.append(wire[off:off + ln])
            off += ln
    lib = g.load()
    rng = random.Random(5)
    bufs = [g.DeviceBuffer(data=s, offset=rng.randrange(16)) for s in slices]
    tx, rx = g.Pair(R, max_sge, 0), g.Pair(R, max_sge, 0)
    g.connect_pairs(tx, rx)
    N = sum(len(s) for s in slices)
    dst_cap = N + 32 * (2 * len(slices) + 64) + 4096
    dst = g.DeviceBuffer(nbytes=dst_cap)
    job = gs.MultiStreamJob([(tx, rx, [(b.ptr, len(s)) for b, s in zip(bufs, slices)], dst.ptr, dst_cap, 2 * len(slices) + 64)], 4096)
    job.set_pipeline(True)
    if sends > 1:
        job.set_sends(sends)
    job.set_promised_credit(True)
    link = _LaggedLink(R, max_sge)
    try:
        r = job.run(gs.RUN_EAGER)   # (a promised-credit job's eager pass runs its rounds in order: every credit seen)
        assert r.done and r.bytes_delivered == N
        exp1, rounds1 = link.sequential_pass(0, slices, sends)
        mem = dst.read(dst_cap)
        assert [mem[o:o + n] for o, n in job.delivered_slices(0)] == exp1
        graph_rounds = 2 * rounds1 + 6
        job.set_rounds(graph_rounds)
        pc0 = _promise_counts(g)
        assert lib.grdma_debug_set_promise_wait(1) == 0
        for _ in range(2):
            r = job.run(gs.RUN_GRAPH)
            assert r.done and r.bytes_delivered == N and r.bytes_sent == N
        assert lib.grdma_debug_set_promise_wait(0) == 0
        pc1 = _promise_counts(g)
        kept, none_, older, ran_out = [b - a for a, b in zip(pc0, pc1)]
        print("graph passes: Sends priced with the promise %d / no credit in the drain %d / older block %d; launches whose "
              "wait ran out %d" % (kept, none_, older, ran_out))
        mem = dst.read(dst_cap)
        got = [mem[o:o + n] for o, n in job.delivered_slices(0)]
        assert b"".join(got) == b"".join(slices)
        assert rx.ring_mem() == bytes(R)
        txs, rxs = tx.state(), rx.state()
        assert rxs["head"] == txs["remote_tail"] and rxs["remain"] == 0
        if os.environ.get("GRDMA_TEST_ALLOW_EMU") != "1":
            assert ran_out >= 1, "the knob did not make any wait run out"
        if ran_out and kept + none_ + older == 0:
            for _ in range(2):
                exp, used = link.paired_pass(0, slices, graph_rounds, sends)
        elif ran_out == 0:
            for _ in range(2):
                exp, _r = link.sequential_pass(0, slices, sends)
        else:
            exp = None   # (some launches kept the promise, some gave it up: each Send is uniform, the pass is a mix)
        if exp is not None:
            assert [len(x) for x in got] == [len(x) for x in exp]
            assert got == exp
            st0, st1 = link.o.state(0), rx_state_of(link.o)
            assert rx.ring_mem() == link.o.ring_mem(1)
            for k in ("remote_tail", "remote_head", "partial_write"):
                assert txs[k] == st0[k], k
            check_rx_state(rxs, st1)
    finally:
        lib.grdma_debug_set_promise_wait(0)
        link.o.close()
        job.close()
        tx.close()
        rx.close()


@pytest.mark.parametrize("promise", [False, True], ids=["credit_a_round_late", "promised_credit"])
@pytest.mark.parametrize("case", [(2, 1 << 18, 30, 5, 65539), (32, 4 << 20, 4095, 64, 65539)], ids=["pairs2_r256k", "pairs32_r4m_bench"])
def test_config3_bidirectional_job_on_every_link_matches_the_oracle(gpu, case, promise):
    """BASELINE configs[3] as bench.py times it (value_conns32_64KiB_bidi): 32 pairs, 4 MiB rings, 64 x 64 KiB messages
    in EACH direction of every pair, all 64 links in every launch of one job on the paired graph -- a ring every round
    fills, so every Send is cut by the credit and the credit arrives a round late.  Every one of the 64 links against
    the oracle driven the same way (a sequential pass, then two passes of the paired chain; pair.cc:264-301,
    rdma_bp_posix.cc:180-291, 470-524): delivered slices, ring image, sender and receiver state.  (bench.py itself
    checks the bytes of the first and the last link only.)
    promised_credit (round 6): the same job with grdma_stream_job_set_promised_credit -- 64 links x (3 + 3) planner
    workgroups are more than the device has CUs, which the mode refused through the first half of the round; dispatch
    order makes it safe (a Send's workgroups get a CU only after every drain workgroup of the launch has one) -- against
    the oracle's PLAIN rounds on every link."""
    from grpc_rdma_amd import stream as gs
    g = gpu
    pairs, R, max_sge, n_msgs, msg_len = case
    links, keep, pr = [], [], []
    for p in range(pairs):
        a, b = g.Pair(R, max_sge, 0), g.Pair(R, max_sge, 0)
        g.connect_pairs(a, b)
        pr.append((a, b))
        for d, (tx, rx) in enumerate(((a, b), (b, a))):
            wire, lens = framed(n_msgs, msg_len, seed=1000 + 2 * p + d)
            sl, off = [], 0
            for n in lens:
                sl.append(wire[off:off + n])
                off += n
            rng = random.Random(7 * p + d)
            packed, offs = bytearray(), []
            for s in sl:
                packed += bytes(rng.randrange(1, 16))
                offs.append(len(packed))
                packed += s
            buf = g.DeviceBuffer(data=bytes(packed) + bytes(64))
            scap = 2 * len(sl) + 64 + len(wire) // 256
            cap = len(wire) + 32 * scap + 4096
            dst = g.DeviceBuffer(nbytes=cap)
            links.append((tx, rx, [(buf.ptr + o, len(s)) for o, s in zip(offs, sl)], dst.ptr, cap, scap))
            keep.append((sl, buf, dst, cap))
    total = sum(sum(len(s) for s in k[0]) for k in keep)
    job = gs.MultiStreamJob(links, 4096)
    job.set_pipeline(False)
    r = job.run(gs.RUN_EAGER)                       # pass 1: sequential rounds
    assert r.done and r.bytes_delivered == total
    rounds1 = int(max(r.tx_rounds, r.rx_rounds))
    graph_rounds = 2 * rounds1 + 6
    job.set_pipeline(True)
    if promise:
        job.set_promised_credit(True)
    job.set_rounds(graph_rounds)
    pc0 = _promise_counts(g)
    for _ in range(2):                              # passes 2, 3: the paired graph, what bench.py times
        r = job.run(gs.RUN_GRAPH)
        assert r.done and r.bytes_delivered == total and r.bytes_sent == total
    used_max = 0
    for p in range(pairs):
        o = _LaggedLink(R, max_sge)
        exp = [None, None]
        for d in (0, 1):
            _e, r1 = o.sequential_pass(d, keep[2 * p + d][0])
            assert r1 <= rounds1
        for _ in range(2):
            for d in (0, 1):   # (the two directions of a pair share no protocol state: driven one after the other)
                if promise:
                    exp[d], used = o.sequential_pass(d, keep[2 * p + d][0])
                else:
                    exp[d], used = o.paired_pass(d, keep[2 * p + d][0], graph_rounds)
                used_max = max(used_max, used)
        a, b = pr[p]
        for d in (0, 1):
            sl, _buf, dst, cap = keep[2 * p + d]
            mem = dst.read(cap)
            got = [mem[o_:o_ + n] for o_, n in job.delivered_slices(2 * p + d)]
            assert [len(x) for x in got] == [len(x) for x in exp[d]], "pair %d direction %d" % (p, d)
            assert got == exp[d], "pair %d direction %d" % (p, d)
        assert a.ring_mem() == o.o.ring_mem(0) == bytes(R) and b.ring_mem() == o.o.ring_mem(1) == bytes(R), "pair %d" % p
        for pair_, s_ in ((a, rx_state_of(o.o, 0)), (b, rx_state_of(o.o, 1))):
            ps = pair_.state()
            for k in ("remote_tail", "remote_head", "partial_write"):
                assert ps[k] == s_[k], (p, k)
            check_rx_state(ps, s_, p)
        o.o.close()
    print("rounds: sequential %d, paired %d of %d" % (rounds1, used_max, graph_rounds))
    if promise:
        pc = [b_ - a_ for a_, b_ in zip(pc0, _promise_counts(g))]
        print("promised-credit Sends: priced with it %d, none in the drain %d, older block %d, waits that ran out %d" % tuple(pc))
        assert pc[3] == 0 and pc[0] > 0, pc
    elif pairs == 2:
        assert used_max > rounds1, "the small configuration was meant to be credit-limited on the paired schedule"
    job.close()
    for a, b in pr:
        a.close()
        b.close()
