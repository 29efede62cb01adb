"""Replies framed on the device from descriptors (grdma_h2_reply) in bench.py's with-h2 shape: 1008 x 1 MiB messages on
stream 1, 16 KiB frames, 256 MiB rings.  A forward pipe with an assembler over one connection, the way back over a
second connection.

Two things are measured, both against the host-table framer on the same box in the same process, alternating:

  framing   grdma_h2_reply_frame over the descriptors of one standalone call (the 1008 messages the forward job
            delivered) against grdma_h2_frame_messages for the same 1008 messages from a host table: HIP-event time
            of the kernels, median of --frames calls each.  An empty launch is taken as half the time of
            grdma_h2_reply_frame over a call without descriptors (its two launches with nothing to do).
  echo      ms per step of forward pipe + reply pipe, against the forward pipe + an independent host-table pipe over
            the same second connection, in alternating rounds of --steps steps; GiB/s counts the user payload of both
            directions.

  python tools/h2_reply_probe.py --out profiles/h2_reply_probe.json
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o t -- python tools/h2_reply_probe.py --reply-only
  python tools/h2_reply_probe.py --merge-stats DIR/..._kernel_stats.csv --out profiles/h2_reply_probe.json

Run every GPU step under a time limit of its own (timeout -k 10 <s> ...) and chain the steps with &&."""
import argparse
import csv
import json
import os
import re
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("k_h2_reply_plan", "k_h2_reply_emit", "k_h2_frame_one", "k_h2_frame_index", "k_h2_frame_emit", "k_h2_asm_copy")


def merge_stats(path, out):
    res = json.load(open(out)) if os.path.exists(out) else {}
    per = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            for k in KERNELS:
                if re.search(r"\b%s\b" % k, row.get("Name", "")):
                    per[k] = {"calls": int(row["Calls"]), "avg_us": float(row["AverageNs"]) / 1e3}
    res["profile"] = {"kernels": per, "stats_csv": os.path.relpath(path, ROOT)}
    json.dump(res, open(out, "w"), indent=1)
    print(json.dumps(res["profile"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--msgs", type=int, default=1008)
    ap.add_argument("--ring-kb", type=int, default=256 * 1024)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--frames", type=int, default=7, help="framing calls per framer (median)")
    ap.add_argument("--reply-only", action="store_true", help="only the echo steps through the reply pipe (profiled run)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--merge-stats", default=None)
    args = ap.parse_args()
    if args.merge_stats:
        merge_stats(args.merge_stats, args.out)
        return
    import torch
    torch.zeros(1, device="cuda")  # (torch's device first: one HIP runtime then serves both)
    torch.cuda.synchronize()
    sys.path.insert(0, ROOT)
    import bench
    import grpc_rdma_amd as g
    from grpc_rdma_amd import h2dev, stream as gs
    g.init(0)
    lib = g.load()
    w = bench.Workload(g, args.msgs)
    ring = args.ring_kb * 1024
    conns = []
    for _ in range(2):
        tx, rx = g.Pair(ring, 4095, 0), g.Pair(ring, 4095, 0)
        g.connect_pairs(tx, rx)
        conns.append((tx, rx))
    scap = len(w.lens) * 2 + 64 + w.N // 256
    dst_cap = w.N + 16 * scap + 4096
    ev_cap = 4 * len(w.lens) + 1024
    msgs = [(w.payload_buf.ptr + i * w.msg_len, w.msg_len, 1, 0) for i in range(w.n_msgs)]
    payload = w.n_msgs * w.msg_len
    keep = []

    def make_job(conn):
        dst = g.DeviceBuffer(nbytes=dst_cap)
        est = max(8, 4 * (w.E // (ring // 2) + 2), 2 * (len(w.lens) // 4095 + 2))
        job = gs.MultiStreamJob([(conn[0], conn[1], w.sge, dst.ptr, dst_cap, scap)], est)
        job.set_pipeline(True)
        job.set_sends(2)
        r = job.run(gs.RUN_EAGER)
        job.set_rounds(int(max(-(-int(r.tx_rounds) // 2), r.rx_rounds)))
        r = job.run(gs.RUN_GRAPH)
        assert r.done and r.bytes_delivered == w.N
        keep.extend([dst, job])
        return job, dst, int(r.bytes_sent)

    def parser():
        p = h2dev.Parser(False)
        assert p.open_streams([1]) == 0
        return p

    step_bytes = w.n_msgs * (-(-w.msg_len // 256) * 256)
    res = {"workload": "%d x %d B messages on stream 1, 16 KiB frames, %d MiB rings, forward pipe with assembler, "
                       "reply over a second connection" % (w.n_msgs, w.msg_len, args.ring_kb >> 10),
           "payload_bytes_per_direction": payload}

    # ---- framing: descriptors against the host table, standalone calls -------------------------------------------
    job_f, dst_f, _ = make_job(conns[0])
    if not args.reply_only:
        p_s = parser()
        arena_s = torch.empty(step_bytes + (4 << 20), dtype=torch.uint8, device="cuda")
        asm_s = h2dev.Assembler(p_s, arena_s, 4 << 20, 4096)
        err, got = p_s.deframe_messages(dst_f.ptr, job_f.delivered_slices(0), asm_s, ev_cap=ev_cap, msgs_cap=4096)
        assert err == 0 and len(got) == w.n_msgs and all(m.status == 0 and m.length == w.msg_len for m in got)
        reply_s = h2dev.Reply(asm_s, None, 16384, 4096)
        cap = len(w.lens) + 64
        sl_buf, hdr_buf = g.DeviceBuffer(nbytes=16 * cap), g.DeviceBuffer(nbytes=32 * cap)
        t_host, t_reply = [], []
        for _ in range(args.frames):
            n, wire = h2dev.frame_messages(msgs, 16384, sl_buf.ptr, cap, hdr_buf.ptr, 32 * cap)
            t_host.append(float(lib.grdma_h2_last_kernel_us()))
            assert n == len(w.lens) and wire == w.N
            n, st = reply_s.frame(sl_buf.ptr, cap, hdr_buf.ptr, 32 * cap)
            t_reply.append(st["frame_us"])
            assert n == len(w.lens) and st["wire_bytes"] == w.N and st["kept"] == w.n_msgs
        # the reply's slice table against the payload it points at: lengths, and the first and last message's bytes
        raw = sl_buf.read(16 * n)
        lens = [int.from_bytes(raw[16 * i + 8:16 * i + 16], "little") for i in range(n)]
        table_ok = lens == w.lens
        for m in (got[0], got[-1]):
            ref = torch.frombuffer(bytearray(w.msgs[got.index(m) % len(w.msgs)]), dtype=torch.uint8).cuda()
            table_ok = table_ok and torch.equal(arena_s[m.offset:m.offset + m.length], ref)
        # a call that finishes no message: the two launches with nothing to do
        asm_s.release(1 << 62)
        empty = g.DeviceBuffer(nbytes=64)
        err, none = p_s.deframe_messages(empty.ptr, [], asm_s, ev_cap=ev_cap, msgs_cap=4096)
        assert err == 0 and none == []
        t_empty = []
        for _ in range(args.frames):
            n0, st = reply_s.frame(sl_buf.ptr, cap, hdr_buf.ptr, 32 * cap)
            assert n0 == 0
            t_empty.append(st["frame_us"])
        host_us, reply_us = statistics.median(t_host), statistics.median(t_reply)
        empty_launch_us = statistics.median(t_empty) / 2
        res["framing"] = {"host_table_us": host_us, "descriptors_us": reply_us, "empty_launch_us": empty_launch_us,
                          "host_table_us_all": t_host, "descriptors_us_all": t_reply, "ratio": reply_us / host_us if host_us else None,
                          "slice_table_equal": bool(table_ok),
                          "within_expectation": bool(reply_us <= max(1.5 * host_us, host_us + empty_launch_us))}
        reply_s.close()
        asm_s.close()
        del arena_s

    # ---- echo steps ----------------------------------------------------------------------------------------------
    p_f = parser()
    fwd = h2dev.Pipe(job_f, msgs, p_f, len(job_f.delivered_slices(0)), ev_cap)
    arena = torch.empty(step_bytes + (4 << 20), dtype=torch.uint8, device="cuda")
    asm = h2dev.Assembler(p_f, arena, 4 << 20, 4096)
    fwd.attach_assembler(asm)
    reply = h2dev.Reply(asm, None, 16384, 4096)
    job_r, dst_r, sent_r = make_job(conns[1])
    p_r = parser()
    rp = h2dev.Pipe.reply(job_r, reply, p_r, len(job_r.delivered_slices(0)), ev_cap, sent_r)
    sets = {"reply": (fwd, rp)}
    if not args.reply_only:
        job_h, dst_h, _ = make_job(conns[1])
        sets["host_table"] = (fwd, h2dev.Pipe(job_h, msgs, parser(), len(job_h.delivered_slices(0)), ev_cap))

    def run(pair, n):
        t0 = time.perf_counter()
        for _ in range(n):
            pair[0].enqueue()
            pair[1].enqueue()
        out = [p.sync() for p in pair]
        return time.perf_counter() - t0, out

    for pair in sets.values():  # warm-up
        run(pair, 2)
    times = {k: [] for k in sets}
    last = {}
    for _ in range(args.rounds):
        for name, pair in sets.items():
            t, last[name] = run(pair, args.steps)
            times[name].append(t)
    ok = all(r["h2_error"] == 0 and r["frame_overflow"] == 0 and r["deframe_overflow"] == 0 for rs in last.values() for r in rs)
    ok = ok and last["reply"][1]["framed"] == len(w.lens) and [ln for _, ln in rp.slice_table(len(w.lens) + 64)] == w.lens
    if "host_table" in last:
        ok = ok and last["reply"][1]["events"] == last["host_table"][1]["events"]
    res.update({"steps_per_round": args.steps, "rounds": args.rounds, "echo_steps_ok": bool(ok)})
    for name, ts in times.items():
        ms = 1e3 * min(ts) / args.steps
        res["step_ms_" + name] = ms
        res["gibps_both_directions_" + name] = 2 * payload / (ms * 1e-3) / (1 << 30)
        res["round_s_" + name] = ts
    if "host_table" in times and "framing" in res:
        res["echo_extra_us_per_step"] = (res["step_ms_reply"] - res["step_ms_host_table"]) * 1e3
        res["framing_extra_us"] = res["framing"]["descriptors_us"] - res["framing"]["host_table_us"]
    print(json.dumps(res))
    if args.out:
        old = json.load(open(args.out)) if os.path.exists(args.out) else {}
        old.update(res)
        json.dump(old, open(args.out, "w"), indent=1)
    rp.close()
    for pair in sets.values():
        pair[1].close()
    reply.close()
    fwd.close()
    asm.close()
    if not ok or ("framing" in res and not res["framing"]["slice_table_equal"]):
        sys.exit(1)


if __name__ == "__main__":
    main()
