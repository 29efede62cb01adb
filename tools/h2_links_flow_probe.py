"""Receive flow control on every link of a multi-connection job (grdma_h2_fc_account_batch, the group pipe with ledgers)
in the shape of tools/h2_links_probe.py: 32 links -- 16 pairs, both directions -- of 64 x 64 KiB messages per link and
step, 16 KiB frames, 4 MiB rings, paired schedule, two rounds of slack.

  (a) account  32 grdma_h2_fc_account calls, one per link (HIP events: sum, slowest, median), against ONE
               grdma_h2_fc_account_batch over 32 twin ledgers on the same deframings.  Expectation, as for the batched
               deframer: the batch takes no more than 1.5 x the slowest single call -- near one transport's time, not the
               sum; its ratio to the sum is recorded beside it.
  (b) pipe     ms per step of the group pipe with ledgers on all links, less the same pipe without them (measured first,
               on the same box).  Expectation: the difference is no more than the five k_h2_links_fc_* kernels under
               rocprofv3 --kernel-trace --stats (a run of its own) plus one empty launch.
  An empty launch is timed between HIP events (grdma_h2_deframe over an empty list).

  python tools/h2_links_flow_probe.py --run --out profiles/h2_links_flow_probe.json

--run is the driver: the measuring step, the kernel-trace step and the merge are child processes, every GPU step under a
time limit of its own (timeout -k 10 <s> ...), and the driver stops at the first non-zero status; nothing is retried.  An
expectation the run did not reach stays "not measured".  The steps by hand:

  python tools/h2_links_flow_probe.py --out profiles/h2_links_flow_probe.json
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o t -- python tools/h2_links_flow_probe.py --profiled
  python tools/h2_links_flow_probe.py --merge-stats DIR/..._kernel_stats.csv --out profiles/h2_links_flow_probe.json"""
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
LINK_KERNELS = ("k_h2_links_fc_clear", "k_h2_links_fc_keys", "k_h2_links_fc_sums", "k_h2_links_fc_finish", "k_h2_links_fc_emit")
KERNELS = LINK_KERNELS + ("k_h2_fc_clear", "k_h2_fc_keys", "k_h2_fc_sums", "k_h2_fc_finish", "k_h2_fc_emit", "k_h2_deframe_links")
EXPECT_A = "expectation_a_batch_within_1.5x_slowest_single"
EXPECT_B = "expectation_b_ledgers_within_five_kernels_plus_empty_launch"


def write(out, res):
    old = json.load(open(out)) if os.path.exists(out) else {}
    old.update(res)
    for k in (EXPECT_A, EXPECT_B):
        old.setdefault(k, "not measured")
    json.dump(old, open(out, "w"), indent=1)
    return old


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
    upd = {"profile": prof}
    if all(k in per for k in LINK_KERNELS):
        five = sum(per[k]["avg_us"] for k in LINK_KERNELS)
        prof["five_links_kernels_us"] = round(five, 1)
        if "ledgers_minus_plain_us" in res and "empty_launch_us" in res:
            budget = five + res["empty_launch_us"]
            prof["ledgers_budget_us"] = round(budget, 1)
            upd[EXPECT_B] = "met" if res["ledgers_minus_plain_us"] <= budget else "missed"
    print(json.dumps(write(out, upd)["profile"]))


def drive(args):
    """every GPU step a child under its own time limit; the first non-zero status ends the run"""
    me = [sys.executable, os.path.abspath(__file__)]
    shape = ["--links", str(args.links), "--msgs", str(args.msgs), "--payload", str(args.payload), "--ring-kb", str(args.ring_kb)]
    out = args.out or os.path.join(ROOT, "profiles", "h2_links_flow_probe.json")
    write(out, {})   # (what no step reaches stays "not measured")
    with tempfile.TemporaryDirectory() as td:
        steps = [["timeout", "-k", "10", "300"] + me + shape + ["--out", out],
                 ["timeout", "-k", "10", "240", "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", td,
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
    ap.add_argument("--calls", type=int, default=7)
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
        args.steps, args.rounds, args.calls = 5, 1, 1
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
    med = statistics.median
    WINDOW = (1 << 31) - 1
    MAXU = 16
    cap = (13 * MAXU + 22) // 23

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
    delivered = [job.delivered_slices(li) for li in range(L)]

    def parsers():
        ps = [h2dev.Parser(False, chunks=False) for _ in range(L)]
        for p in ps:
            assert p.open_streams([1]) == 0
        return ps

    def ledgers(ps):
        return [h2dev.FlowControl(p, stream_window=WINDOW, conn_window=WINDOW, conn_threshold=0, max_updates=MAXU) for p in ps]

    def good(res, what):
        # the connection's frame and stream 1's; every DATA byte counted for both
        assert res[0] == 2 and res[7] == 0 and res[5] == 0 and res[3] == res[4] > w0.msg_len * args.msgs, (what, res)

    res = {"workload": "%d links (%d pairs, both directions) x %d x %d B messages per step on stream 1, 16 KiB frames, "
                       "%d KiB rings, paired schedule" % (L, L // 2, args.msgs, w0.msg_len, args.ring_kb)}

    # ---- (a) the same deframings accounted 32 x 1 and 1 x 32 (twin parsers: a ledger accounts a deframing once)
    ps_1, ps_b = parsers(), parsers()
    fc_1, fc_b = ledgers(ps_1), ledgers(ps_b)
    tg = [(g.DeviceBuffer(nbytes=16 * cap), g.DeviceBuffer(nbytes=32 * cap)) for _ in range(2 * L)]
    rows, batch = [], []
    for call in range(args.calls + 2):
        for li in range(L):
            for ps in (ps_1, ps_b):
                err, _ = ps[li].deframe(dsts[li].ptr, delivered[li], cap=ev_cap)
                assert err == 0
        row = []
        for li in range(L):
            _, r1, _ = fc_1[li].account(tg[li][0].ptr, cap, tg[li][1].ptr, 32 * cap)
            good(r1, ("single", li))
            row.append(fc_1[li].stats()["kernel_us"])
        rows.append(row)
        out = h2dev.account_batch([(fc_b[li], tg[L + li][0].ptr, cap, tg[L + li][1].ptr, 32 * cap) for li in range(L)])
        for li, (_, rb, _) in enumerate(out):
            good(rb, ("batch", li))
            assert rb == fc_1[li].last_result, li
        batch.append(fc_b[0].stats()["kernel_us"])
    single = [med(r[li] for r in rows[2:]) for li in range(L)]
    b_us = med(batch[2:])
    res["single_calls_account_us"] = {"sum": round(sum(single), 1), "slowest": round(max(single), 1), "median": round(med(single), 1)}
    res["batch_account_us"] = round(b_us, 1)
    res["batch_over_slowest_single"] = round(b_us / max(single), 2)
    res["batch_over_sum_of_singles"] = round(b_us / sum(single), 3)
    res[EXPECT_A] = "met" if b_us <= 1.5 * max(single) else "missed"
    empty = []
    for _ in range(args.calls + 2):
        ps_1[0].deframe(dsts[0].ptr, [], cap=64)
        empty.append(float(lib.grdma_h2_last_kernel_us()))
    res["empty_launch_us"] = round(med(empty[2:]), 1)
    for f in fc_1 + fc_b:
        f.close()

    # ---- (b) the group pipe's step without and with ledgers on all links
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

    ps = parsers()
    specs = []
    for li, w in enumerate(wls):
        msgs = [(w.payload_buf.ptr + i * w.msg_len, w.msg_len, 1, 0) for i in range(w.n_msgs)]
        specs.append((li, msgs, ps[li], len(delivered[li]), ev_cap))
    gp = h2dev.GroupPipe(job, specs)

    def step_ok(with_fc):
        rs = gp.sync()
        assert all(x["h2_error"] == 0 and x["deframe_overflow"] == 0 and x["frame_overflow"] == 0 for x in rs), rs
        if with_fc:
            for li in range(L):
                good(gp.window_updates(li)[1], ("pipe", li))

    for _ in range(2):
        gp.enqueue()
        step_ok(False)
    ms_plain = timed(gp.enqueue, gp.sync)
    step_ok(False)
    fcs = ledgers(ps)   # (the pipe refuses a parser that has a ledger when it is created: the ledgers come behind it)
    gp.attach_flow_control(fcs)
    res["hook_counts_group_pipe_with_ledgers"] = list(gp.hook_counts())
    for _ in range(2):
        gp.enqueue()
        step_ok(True)
    ms_fc = timed(gp.enqueue, gp.sync)
    step_ok(True)
    gp.close()
    for f in fcs:
        f.close()
    res["pipe_ms_per_step"] = {"with_ledgers": [round(x, 4) for x in ms_fc], "plain": [round(x, 4) for x in ms_plain]}
    res["ledgers_minus_plain_us"] = round((med(ms_fc) - med(ms_plain)) * 1e3, 1)
    res["ledgers_budget_hip_events_us"] = round(b_us + res["empty_launch_us"], 1)   # (the kernel trace's sum comes with --merge-stats)
    print(json.dumps(res))
    if args.out:
        write(args.out, res)
    return 0


if __name__ == "__main__":
    sys.exit(main())
