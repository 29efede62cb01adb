"""What the device tests of the streaming job share (tests/test_gpu_stream_job.py, tests/test_gpu_bench_configs.py,
tests/planner_sweep_lib.py, tools/promise_probe.py): framed messages as chttp2 hands them to the endpoint, one job run
three times over a list of slices with what it left behind, the receive state against the oracle's, the rdma_flush
cursor, and the library's planner counters."""
import random

from oracle import pyorc

PASSES = 3  # the job is run three times on the same connection (eager, graph, graph)


RX_KEYS = ("head", "moving_head", "remain", "internal_read_size", "credit_msgs", "leftover_cap")


def framed(n_msgs, msg_len, seed, max_frame=16384):
    """-> (wire bytes, slice lengths) of n_msgs framed messages as chttp2 hands them to the endpoint;
    message i is a rotation of one random block, so every message differs."""
    rng = random.Random(seed)
    block = bytes(rng.getrandbits(8) for _ in range(4099))
    wire, lens = bytearray(), []
    for i in range(n_msgs):
        rot = (i * 131) % len(block)
        body = (block[rot:] + block[:rot]) * (msg_len // len(block) + 1)
        w, l = pyorc.h2_frame_message(body[:msg_len], stream_id=2 * i + 1, max_frame=max_frame)
        wire += w
        lens += l
    return bytes(wire), lens


def rx_state_of(o, side=1):
    """The oracle's state of one side with the capacity of the read its last would-block left open beside it
    (pyorc.OracleLink.state() does not carry leftover_cap)."""
    return dict(o.state(side), leftover_cap=int(o.p[side].leftover_cap))


def check_rx_state(got, exp, tag=None, total_read=None):
    """What a drain's commit leaves in the connection, against the oracle: every key of RX_KEYS that `exp` holds (a dict
    of rx_state_of), and total_read against the payload bytes the caller knows the passes delivered."""
    for k in RX_KEYS:
        if k in exp:
            assert got[k] == exp[k], (k, got[k], exp[k], tag)
    if total_read is not None:
        assert got["total_read"] == total_read, ("total_read", got["total_read"], total_read, tag)


def _run_job(g, R, max_sge, slices, pipeline, flags=0, mode=None, sends=1, promise=False, fused_wire=None, pairs=None, more_passes=()):
    """pairs: a connected (tx, rx) the caller keeps (pairs taken from the PairPool: tests/planner_sweep_lib.py); they are
    left open.  more_passes: passes behind the usual three -- a run mode, or "streams" for launch(streams=True) + sync();
    out["more"] holds slices, ring, state and timed classes after each of them."""
    from grpc_rdma_amd import stream as gs
    rng = random.Random(5)
    bufs = [g.DeviceBuffer(data=s, offset=rng.randrange(16)) for s in slices]
    if pairs is not None:
        tx, rx = pairs
    else:
        tx, rx = g.Pair(R, max_sge, flags), g.Pair(R, max_sge, flags)
        g.connect_pairs(tx, rx)
    N = sum(len(s) for s in slices)
    dst_cap = N + 32 * (2 * len(slices) + 64) + 4096
    dst = g.DeviceBuffer(nbytes=dst_cap)
    sge = [(b.ptr, len(s)) for b, s in zip(bufs, slices)]
    # (an eager run launches every round it was given, also the ones that find nothing to do: a bound from the sizes
    # instead of 4096 -- rounds are cut by the staging budget, R / 2, or by max_sge, whichever comes first)
    bound = min(4096, 6 * (N // (R // 2) + len(slices) // max_sge) + 24)
    job = gs.MultiStreamJob([(tx, rx, sge, dst.ptr, dst_cap, 2 * len(slices) + 64)], bound)
    job.set_pipeline(pipeline)
    if sends > 1:
        job.set_sends(sends)
    if promise:
        job.set_promised_credit(True)
    if fused_wire is not None:
        job.set_fused_wire(fused_wire)
    r = job.run(gs.RUN_EAGER)
    assert r.done and r.bytes_delivered == N and r.bytes_sent == N
    rounds = int(max(r.tx_rounds, r.rx_rounds))  # (tx_rounds counts Sends: an upper bound of the rounds)
    # replay as a captured graph; later passes start at another ring phase and may need a
    # round more or less than the first (surplus rounds find nothing to do).  With a
    # small ring the pipelined sender can also meet a round in which the credit of the
    # round before has not landed yet and nothing fits: leave room for those.
    job.set_rounds(2 * rounds + 4 if pipeline else rounds + 2)
    for i in range(PASSES - 1):
        r = job.run(mode if (mode is not None and i == PASSES - 2) else gs.RUN_GRAPH)
        assert r.done and r.bytes_delivered == N and r.bytes_sent == N
    def snapshot(last):
        ds = job.delivered_slices(0)
        mem = dst.read(dst_cap)
        return {"slices": [mem[o:o + n] for o, n in ds], "ring": rx.ring_mem(), "tx": tx.state(), "rx": rx.state(),
                "launches": [int(x) for x in last.launches_class] if last else None,
                "ms": [float(x) for x in last.ms_class] if last else None}
    out = snapshot(r)
    out.update({"rounds": rounds, "wire_groups": job.wire_groups(), "rounds_set": 2 * rounds + 4 if pipeline else rounds + 2, "more": []})
    for m in more_passes:
        if m == "streams":
            job.launch(streams=True)
            job.sync()
            out["more"].append(snapshot(None))
        else:
            r = job.run(m)
            assert r.done and r.bytes_delivered == N and r.bytes_sent == N
            out["more"].append(snapshot(r))
    job.close()
    if pairs is None:
        tx.close()
        rx.close()
    return out


def _table_cache_stats(g):
    import ctypes as C
    lib = g.load()
    out = (C.c_uint64 * 2)()
    assert lib.grdma_rx_table_cache_stats(out) == 0
    return [int(x) for x in out]


def _fast_counts(g):
    import ctypes as C
    lib = g.load()
    out = (C.c_uint64 * 6)()
    assert lib.grdma_rx_fast_drains(out) == 0
    tx = (C.c_uint64 * 2)()
    assert lib.grdma_tx_fast_sends(tx) == 0
    return [int(x) for x in out] + [int(x) for x in tx]


def _advance(slices, idx, byte, sent):
    left = sent
    while left > 0:  # the rdma_flush cursor, rdma_bp_posix.cc:480-493
        room = len(slices[idx]) - byte
        if left >= room:
            left -= room
            idx += 1
            byte = 0
        else:
            byte += left
            left = 0
    return idx, byte
