"""HTTP/2 on every link of a multi-connection job (grdma_h2_group_pipe, grdma_h2_deframe_batch) in the shape of
bench.py's value_conns32_64KiB_bidi leg: 32 links -- 16 pairs, both directions -- of 64 x 64 KiB messages per step,
16 KiB frames, 4 MiB rings, paired schedule.

  (a) ms per step of the job with the group pipe (k_h2_frame_links + k_h2_deframe_links inside its graph);
  (b) ms per step of the same job carrying the same framed slice tables without any kernel of HTTP/2 (tables framed
      once, up front, on the host: bench.Workload);  (a) - (b) is what the two stages cost inside the graph;
  (c) the 32 links' delivered slices deframed by 32 grdma_h2_deframe calls: HIP-event kernel time of each, their sum
      and the slowest;
  (d) the same slices by one grdma_h2_deframe_batch: HIP-event time of the launch, median of --calls calls.
  An empty launch is timed between HIP events the same way (grdma_h2_deframe over an empty list: one workgroup that
  reads its parser block and leaves).

  python tools/h2_links_probe.py --out profiles/h2_links_probe.json
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o t -- python tools/h2_links_probe.py --profiled
  python tools/h2_links_probe.py --merge-stats DIR/..._kernel_stats.csv --out profiles/h2_links_probe.json

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
KERNELS = ("k_h2_frame_links", "k_h2_deframe_links", "k_h2_deframe", "k_h2_frame_one")


def merge_stats(path, out):
    res = json.load(open(out)) if os.path.exists(out) else {}
    per = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            for k in KERNELS:
                if re.search(r"\b%s\b" % k, row.get("Name", "")):
                    per[k] = {"calls": int(row["Calls"]), "avg_us": float(row["AverageNs"]) / 1e3,
                              "min_us": float(row["MinNs"]) / 1e3, "max_us": float(row["MaxNs"]) / 1e3}
    res["profile"] = {"kernels": per, "stats_csv": os.path.basename(path)}
    json.dump(res, open(out, "w"), indent=1)
    print(json.dumps(res["profile"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--links", type=int, default=32)
    ap.add_argument("--msgs", type=int, default=64, help="messages per link and step (bench.py: max(8, 2048 // 32))")
    ap.add_argument("--payload", type=int, default=64 * 1024)
    ap.add_argument("--ring-kb", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5, help="timed regions of --steps steps per variant (median)")
    ap.add_argument("--calls", type=int, default=9, help="deframing calls per variant (median)")
    ap.add_argument("--profiled", action="store_true", help="few steps and calls: the run under rocprofv3")
    ap.add_argument("--out", default=None)
    ap.add_argument("--merge-stats", default=None)
    args = ap.parse_args()
    if args.merge_stats:
        merge_stats(args.merge_stats, args.out)
        return
    if args.profiled:
        args.steps, args.rounds, args.calls = 5, 1, 7
    import torch
    torch.zeros(1, device="cuda")  # (torch's device first: one HIP runtime then serves both)
    torch.cuda.synchronize()
    sys.path.insert(0, ROOT)
    import bench
    import grpc_rdma_amd as g
    from grpc_rdma_amd import h2dev, stream as gs
    g.init(0)
    lib = g.load()
    L, ring = args.links, args.ring_kb * 1024
    assert L % 2 == 0
    wls = [bench.Workload(g, args.msgs, args.payload, stream_id=1) for _ in range(L)]
    w0 = wls[0]
    scap = len(w0.lens) * 2 + 64 + w0.N // 256
    dst_cap = w0.N + 16 * scap + 4096
    ev_cap = 4 * len(w0.lens) + 1024
    user_bytes = L * args.msgs * args.payload

    def make_job():
        links, dsts, prev = [], [], None
        for k, w in enumerate(wls):
            if k % 2 == 1:
                rx, tx = prev       # the other direction over the same two ends
            else:
                tx, rx = g.Pair(ring, 4095, 0), g.Pair(ring, 4095, 0)
                g.connect_pairs(tx, rx)
                prev = (tx, rx)
            dst = g.DeviceBuffer(nbytes=dst_cap)
            links.append((tx, rx, w.sge, dst.ptr, dst_cap, scap))
            dsts.append(dst)
        est = max(8, 4 * (w0.E // (ring // 2) + 2), 2 * (len(w0.lens) // 4095 + 2))
        job = gs.MultiStreamJob(links, est)
        job.set_pipeline(True)
        r = job.run(gs.RUN_EAGER)
        assert r.done
        # (two rounds of slack: later steps start at another ring phase and may need a round more)
        job.set_rounds(int(max(r.tx_rounds, r.rx_rounds)) + 2)
        r = job.run(gs.RUN_GRAPH)
        assert r.done and r.bytes_delivered == L * w0.N
        return job, dsts, links

    def timed(step, sync):
        for _ in range(3):
            step()
        sync()
        out = []
        for _ in range(args.rounds):
            t0 = time.perf_counter()
            for _ in range(args.steps):
                step()
            sync()
            out.append((time.perf_counter() - t0) / args.steps * 1e3)
        return out

    res = {"workload": "%d links (%d pairs, both directions) x %d x %d B messages per step on stream 1, 16 KiB frames, "
                       "%d KiB rings, paired schedule" % (L, L // 2, args.msgs, w0.msg_len, args.ring_kb),
           "user_payload_bytes_per_step": user_bytes, "published_leg_GiBps": "501-520 (value_conns32_64KiB_bidi)"}

    # (b) the job alone over the framed tables: bench.Workload's slice lists ARE the framed tables (host mirror of the
    # framing); checked against the device framer's lengths below
    job_b, dsts_b, links_b = make_job()   # (the links hold the pairs)
    ms_b = timed(lambda: job_b.launch(), job_b.sync)
    res["job_only_ms_per_step"] = ms_b
    delivered = [job_b.delivered_slices(li) for li in range(L)]

    # (c) / (d) the delivered slices of the 32 links, standalone
    def parsers():
        ps = [h2dev.Parser(False, chunks=False) for _ in range(L)]
        for p in ps:
            assert p.open_streams([1]) == 0
        return ps

    ps_c, ps_d, p_e = parsers(), parsers(), parsers()[:1]
    singles = []
    for _ in range(args.calls):
        row = []
        for li in range(L):
            err, ev = ps_c[li].deframe(dsts_b[li].ptr, delivered[li], cap=ev_cap)
            assert err == 0 and sum(1 for e in ev if e[0] == 5) == args.msgs
            row.append(float(lib.grdma_h2_last_kernel_us()))
        singles.append(row)
    singles = singles[2:] if len(singles) > 4 else singles   # (warm-up)
    per_link = [statistics.median(r[li] for r in singles) for li in range(L)]
    res["single_calls_us"] = {"sum": round(sum(per_link), 1), "slowest": round(max(per_link), 1),
                              "median": round(statistics.median(per_link), 1)}
    batch = []
    for _ in range(args.calls + 2):
        got = h2dev.deframe_batch([(ps_d[li], dsts_b[li].ptr, delivered[li]) for li in range(L)], caps=[ev_cap] * L)
        assert all(err == 0 and sum(1 for e in ev if e[0] == 5) == args.msgs for err, ev in got)
        batch.append(float(lib.grdma_h2_last_kernel_us()))
    batch = batch[2:]
    empty = []
    for _ in range(args.calls + 2):
        p_e[0].deframe(dsts_b[0].ptr, [], cap=64)
        empty.append(float(lib.grdma_h2_last_kernel_us()))
    empty = empty[2:]
    b_us, e_us = statistics.median(batch), statistics.median(empty)
    res["batch_call_us"] = {"median": round(b_us, 1), "all": [round(x, 1) for x in batch]}
    res["empty_launch_us"] = round(e_us, 1)
    res["batch_over_slowest_single"] = round(b_us / max(per_link), 2)
    res["batch_over_sum_of_singles"] = round(b_us / sum(per_link), 3)
    res["expectation_batch_within_1.5x_slowest_single"] = "met" if b_us <= 1.5 * max(per_link) else "missed"

    b = statistics.median(ms_b)
    res["job_only_GiBps_user_payload"] = round(user_bytes / (b * 1e-3) / (1 << 30), 1)

    # (a) the same shape with the group pipe.  A step starts at another ring phase than the recorded run and may deliver
    # a slice more or less (a record cut at the wrap): the pipe parses the step's own count, checked here every step
    job_a, dsts_a, links_a = make_job()
    ps_a = parsers()
    specs = []
    for li, w in enumerate(wls):
        msgs = [(w.payload_buf.ptr + i * w.msg_len, w.msg_len, 1, 0) for i in range(w.n_msgs)]
        specs.append((li, msgs, ps_a[li], len(job_a.delivered_slices(li)), ev_cap))
    gp = h2dev.GroupPipe(job_a, specs)
    counts = set()
    for _step in range(4):
        gp.enqueue()
        r = gp.sync()
        now = [len(job_a.delivered_slices(li)) for li in range(L)]
        counts.update(now)
        assert all(x["frame_overflow"] == 0 and x["framed"] == len(w0.lens) and x["h2_error"] == 0 and
                   x["deframe_overflow"] == 0 for x in r), r
        assert [x["parsed"] for x in r] == now, ([x["parsed"] for x in r], now)
        assert [sum(1 for e in gp.events(li) if e[0] == 5) for li in (0, 1, L - 1)] == [args.msgs] * 3
    assert [n for _, n in gp.slice_table(0)] == w0.lens
    res["delivered_slices_per_link"] = {"recorded_run": specs[0][3], "seen_in_steps": sorted(counts)}
    ms_a = timed(gp.enqueue, gp.sync)
    r = gp.sync()
    assert all(x["h2_error"] == 0 and x["deframe_overflow"] == 0 for x in r)
    assert sum(1 for e in gp.events(L - 1) if e[0] == 5) == args.msgs
    res["group_pipe_ms_per_step"] = ms_a
    a = statistics.median(ms_a)
    res["group_pipe_GiBps_user_payload"] = round(user_bytes / (a * 1e-3) / (1 << 30), 1)
    res["stages_in_graph_us"] = round((a - b) * 1e3, 1)
    gp.close()
    # the two kernels alone: a pipe created with GRDMA_H2_PIPE_FUSED=0 times its stages between HIP events
    fused_env = os.environ.get("GRDMA_H2_PIPE_FUSED")
    os.environ["GRDMA_H2_PIPE_FUSED"] = "0"
    try:
        gp = h2dev.GroupPipe(job_a, specs)
    finally:
        if fused_env is None:
            os.environ.pop("GRDMA_H2_PIPE_FUSED")
        else:
            os.environ["GRDMA_H2_PIPE_FUSED"] = fused_env
    f_us, d_us = [], []
    for _call in range(args.calls + 2):
        gp.enqueue()
        r = gp.sync()
        assert all(x["h2_error"] == 0 for x in r)
        f_us.append(r[0]["frame_us"])
        d_us.append(r[0]["deframe_us"])
    gp.close()
    fr, de = statistics.median(f_us[2:]), statistics.median(d_us[2:])
    res["unfused_stage_us_hip_events"] = {"frame_links": fr, "deframe_links": de}
    res["stages_budget_us"] = round(b_us + fr + e_us, 1)   # batch deframe + framing kernel + one empty launch
    res["expectation_stages_within_budget"] = "met" if res["stages_in_graph_us"] <= res["stages_budget_us"] else "missed"
    del links_a   # (the pairs live as long as the jobs: MultiStreamJob holds them too)
    print(json.dumps(res))
    if args.out:
        old = json.load(open(args.out)) if os.path.exists(args.out) else {}
        old.update(res)
        json.dump(old, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
