"""Replies on every link of a multi-connection job (grdma_h2_reply_frame_batch, the group reply pipe) in the shape of
tools/h2_links_probe.py: 32 links -- 16 pairs, both directions -- of 64 x 64 KiB messages per link and step, 16 KiB
frames, 4 MiB rings, paired schedule, two rounds of slack.

  (a) framing  32 grdma_h2_reply_frame calls, one per link (HIP events: sum, slowest, median), against ONE
               grdma_h2_reply_frame_batch over the 32 links.  Expectation, as for the batched deframer: the batch takes
               no more than 1.5 x the slowest single call -- near one transport's time, not the sum; its ratio to the
               sum is recorded beside it.
  (b) echo     ms per step of forward group pipe (assemblers on all links) + group reply pipe over a back job, less the
               same two jobs with the back job's tables framed from host message tables (an ordinary group pipe).
               Expectation: the difference is no more than k_h2_reply_plan_links + k_h2_reply_emit_links under
               rocprofv3 --kernel-trace --stats (a run of its own) plus one empty launch.
  An empty launch is timed between HIP events (grdma_h2_deframe over an empty list).

  python tools/h2_links_reply_probe.py --run --out profiles/h2_links_reply_probe.json

--run is the driver: the measuring step, the kernel-trace step and the merge are child processes, every GPU step under a
time limit of its own (timeout -k 10 <s> ...), and the driver stops at the first non-zero status.  The steps by hand:

  python tools/h2_links_reply_probe.py --out profiles/h2_links_reply_probe.json
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o t -- python tools/h2_links_reply_probe.py --profiled
  python tools/h2_links_reply_probe.py --merge-stats DIR/..._kernel_stats.csv --out profiles/h2_links_reply_probe.json"""
import argparse
import csv
import glob
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("k_h2_reply_plan_links", "k_h2_reply_emit_links", "k_h2_reply_plan", "k_h2_reply_emit", "k_h2_frame_links")
ALL = 1 << 63


def merge_stats(path, out):
    res = json.load(open(out)) if os.path.exists(out) else {}
    per = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            for k in KERNELS:
                if re.search(r"\b%s\b" % k, row.get("Name", "")):
                    per[k] = {"calls": int(row["Calls"]), "avg_us": float(row["AverageNs"]) / 1e3,
                              "min_us": float(row["MinNs"]) / 1e3, "max_us": float(row["MaxNs"]) / 1e3}
    prof = {"kernels": per, "stats_csv": os.path.basename(path)}
    if "k_h2_reply_plan_links" in per and "k_h2_reply_emit_links" in per:
        two = per["k_h2_reply_plan_links"]["avg_us"] + per["k_h2_reply_emit_links"]["avg_us"]
        prof["two_links_kernels_us"] = round(two, 1)
        if "echo_minus_host_tables_us" in res:
            budget = two + res["empty_launch_us"]
            prof["echo_budget_us"] = round(budget, 1)
            res["expectation_b_echo_within_two_kernels_plus_empty_launch"] = \
                "met" if res["echo_minus_host_tables_us"] <= budget else "missed"
    res["profile"] = prof
    json.dump(res, open(out, "w"), indent=1)
    print(json.dumps(res["profile"]))


def drive(args):
    """every GPU step a child under its own time limit; the first non-zero status ends the run"""
    me = [sys.executable, os.path.abspath(__file__)]
    shape = ["--links", str(args.links), "--msgs", str(args.msgs), "--payload", str(args.payload), "--ring-kb", str(args.ring_kb)]
    out = args.out or os.path.join(ROOT, "profiles", "h2_links_reply_probe.json")
    with tempfile.TemporaryDirectory() as td:
        steps = [["timeout", "-k", "10", "420"] + me + shape + ["--out", out],
                 ["timeout", "-k", "10", "300", "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", td,
                  "-o", "t", "--"] + me + shape + ["--profiled"]]
        for cmd in steps:
            rc = subprocess.call(cmd, cwd=ROOT)
            if rc != 0:
                print("step failed with status %d: %s" % (rc, " ".join(cmd)), file=sys.stderr)
                return rc
        found = glob.glob(os.path.join(td, "**", "*kernel_stats.csv"), recursive=True)
        if not found:
            print("no kernel_stats.csv under %s" % td, file=sys.stderr)
            return 1
        merge_stats(found[0], out)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--links", type=int, default=32)
    ap.add_argument("--msgs", type=int, default=64)
    ap.add_argument("--payload", type=int, default=64 * 1024)
    ap.add_argument("--ring-kb", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=9)
    ap.add_argument("--profiled", action="store_true", help="few steps and calls: the run under rocprofv3")
    ap.add_argument("--run", action="store_true", help="drive all steps as child processes under time limits")
    ap.add_argument("--out", default=None)
    ap.add_argument("--merge-stats", default=None)
    args = ap.parse_args()
    if args.merge_stats:
        merge_stats(args.merge_stats, args.out)
        return 0
    if args.run:
        return drive(args)
    if args.profiled:
        args.steps, args.rounds, args.calls = 5, 1, 3
    if not os.environ.get("GRDMA_LIB_PATH"):   # (a dry run of the script over the emulated library has no device)
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
    gran = (w0.msg_len + 255) // 256 * 256
    arena_bytes = 2 * args.msgs * gran
    bodies = [w0.msgs[i % len(w0.msgs)] for i in range(args.msgs)]
    med = statistics.median

    def multi_job():
        """a job of L links, 16 pairs both ways, recorded over the workload's slice lists (the echo has the same shape)"""
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
        job.set_rounds(int(max(r.tx_rounds, r.rx_rounds)) + 2)   # (two rounds of slack)
        r = job.run(gs.RUN_GRAPH)
        assert r.done and r.bytes_delivered == L * w0.N
        return job, dsts, [job.delivered_slices(li) for li in range(L)]

    def parsers():
        ps = [h2dev.Parser(False, chunks=False) for _ in range(L)]
        for p in ps:
            assert p.open_streams([1]) == 0
        return ps

    def assemblers(ps):
        arenas = [g.DeviceBuffer(nbytes=arena_bytes) for _ in ps]
        return [h2dev.Assembler(p, a, max_pending=max(4096, 2 * args.msgs)) for p, a in zip(ps, arenas)], arenas

    def good(msgs, asm, deep):
        assert len(msgs) == args.msgs and all(m.status == 0 and m.length == w0.msg_len for m in msgs), len(msgs)
        if deep:
            assert all(asm.view(m) == bodies[k % args.msgs] for k, m in enumerate(msgs))

    job_f, dsts_f, delivered_f = multi_job()
    res = {"workload": "%d links (%d pairs, both directions) x %d x %d B messages per step on stream 1, 16 KiB frames, "
                       "%d KiB rings, paired schedule" % (L, L // 2, args.msgs, w0.msg_len, args.ring_kb)}

    # ---- (a) framing: the messages of every link assembled once, then framed 32 x 1 and 1 x 32
    ps_s = parsers()
    as_s, keep_s = assemblers(ps_s)
    got = h2dev.deframe_messages_batch([(ps_s[li], as_s[li], dsts_f[li].ptr, delivered_f[li]) for li in range(L)],
                                       ev_caps=[ev_cap] * L)
    for li, (err, msgs) in enumerate(got):
        assert err == 0
        good(msgs, as_s[li], li in (0, L - 1))
    replies = [h2dev.Reply(a, None, 16384, 2 * args.msgs) for a in as_s]
    cap = len(w0.lens) + 8
    tg = [(g.DeviceBuffer(nbytes=16 * cap), g.DeviceBuffer(nbytes=32 * cap)) for _ in range(L)]
    rows = []
    for call in range(args.calls + 2):
        row = []
        for li in range(L):
            n, st = replies[li].frame(tg[li][0].ptr, cap, tg[li][1].ptr, 32 * cap)
            assert n == len(w0.lens) and st["kept"] == args.msgs and st["wire_bytes"] == w0.N, (n, st)
            row.append(st["frame_us"])
        rows.append(row)
    single = [med(r[li] for r in rows[2:]) for li in range(L)]
    batch = []
    items = [(replies[li], tg[li][0].ptr, cap, tg[li][1].ptr, 32 * cap) for li in range(L)]
    for call in range(args.calls + 2):
        out = h2dev.reply_frame_batch(items)
        assert all(n == len(w0.lens) and st["wire_bytes"] == w0.N for n, st in out)
        batch.append(out[0][1]["frame_us"])
    b_us = med(batch[2:])
    res["single_calls_frame_us"] = {"sum": sum(single), "slowest": max(single), "median": med(single)}
    res["batch_frame_us"] = b_us
    res["batch_over_slowest_single"] = round(b_us / max(single), 2)
    res["batch_over_sum_of_singles"] = round(b_us / sum(single), 3)
    res["expectation_a_batch_within_1.5x_slowest_single"] = "met" if b_us <= 1.5 * max(single) else "missed"
    empty = []
    for _ in range(args.calls + 2):
        ps_s[0].deframe(dsts_f[0].ptr, [], cap=64)
        empty.append(float(lib.grdma_h2_last_kernel_us()))
    res["empty_launch_us"] = round(med(empty[2:]), 1)
    for r in replies:
        r.close()

    # ---- (b) the echo step: forward group pipe with assemblers, then the back job framed from descriptors / from host tables
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

    job_b, dsts_b, delivered_b = multi_job()
    ps_f, ps_b = parsers(), parsers()
    as_f, keep_f = assemblers(ps_f)
    specs = []
    for li, w in enumerate(wls):
        msgs = [(w.payload_buf.ptr + i * w.msg_len, w.msg_len, 1, 0) for i in range(w.n_msgs)]
        specs.append((li, msgs, ps_f[li], len(delivered_f[li]), ev_cap))
    gp = h2dev.GroupPipe(job_f, specs)
    gp.attach_assemblers(as_f)
    replies = [h2dev.Reply(a, None, 16384, 2 * args.msgs) for a in as_f]
    rp = h2dev.GroupPipe.reply(job_b, [(li, replies[li], ps_b[li], len(delivered_b[li]), ev_cap, w0.N) for li in range(L)])
    res["hook_counts_reply_group_pipe"] = list(rp.hook_counts())

    def both_ok(back):
        rf, rb = gp.sync(), back.sync()
        assert all(x["h2_error"] == 0 and x["deframe_overflow"] == 0 and x["frame_overflow"] == 0 for x in rf), rf
        assert all(x["h2_error"] == 0 and x["deframe_overflow"] == 0 and x["frame_overflow"] == 0 for x in rb), rb
        assert all(x["framed"] == len(w0.lens) for x in rb)
        for li in range(L):
            good(gp.messages(li), as_f[li], li in (0, L - 1))
            ends = [e for e in back.events(li) if e[0] == 5]   # EV_MSG_END per echoed message
            assert len(ends) == args.msgs, (li, len(ends))

    def echo_step():
        gp.enqueue()
        rp.enqueue()

    for _ in range(3):
        echo_step()
        both_ok(rp)
    ms_echo = timed(echo_step, lambda: (gp.sync(), rp.sync()))
    both_ok(rp)
    rp.close()
    bspecs = []
    for li, w in enumerate(wls):
        msgs = [(w.payload_buf.ptr + i * w.msg_len, w.msg_len, 1, 0) for i in range(w.n_msgs)]
        bspecs.append((li, msgs, ps_b[li], len(delivered_b[li]), ev_cap))
    hp = h2dev.GroupPipe(job_b, bspecs)

    def host_step():
        gp.enqueue()
        hp.enqueue()

    for _ in range(2):
        host_step()
        both_ok(hp)
    ms_host = timed(host_step, lambda: (gp.sync(), hp.sync()))
    both_ok(hp)
    hp.close()
    gp.close()
    res["echo_ms_per_step"] = {"reply_group_pipe": ms_echo, "host_tables": ms_host}
    res["echo_minus_host_tables_us"] = round((med(ms_echo) - med(ms_host)) * 1e3, 1)
    res["echo_budget_hip_events_us"] = round(b_us + res["empty_launch_us"], 1)   # (the kernel trace's sum comes with --merge-stats)
    for r in replies:
        r.close()
    for x in as_f + as_s:
        x.close()
    print(json.dumps(res))
    if args.out:
        old = json.load(open(args.out)) if os.path.exists(args.out) else {}
        old.update(res)
        json.dump(old, open(args.out, "w"), indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
