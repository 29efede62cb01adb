"""Receive flow control on the device (the window ledger, grdma_h2_fc) in bench.py's with-h2 shape: 1008 x 1 MiB
messages on stream 1, 16 KiB frames, 256 MiB rings, a forward pipe with an assembler, two alternating pipes.

  (a) account   grdma_h2_fc_account alone over the events of one standalone deframing of a step's delivered slices:
                HIP-event time of its five kernels (grdma_h2_fc_stats), median of 7 after two warm-ups, beside one
                empty launch: a one-element kernel (x.add_(0) on a one-byte tensor) between two events on torch's
                stream, median of 101 after warm-up.  (idle_account_us, the account over a call without events, is
                reported too: five launches that still clear and scan the slot table, NOT five empty launches.)
  (b) pipe      ms per step of the pipes with a ledger attached to each, and of the same pipes without (--step
                pipe-base; that step touches nothing of the ledger's API, so tools/ab_builds.sh can run it at the
                parent commit too: alternate the two builds on one box and put the parent's figure in with
                --parent-ms).  Expectation: the difference is at most the ledger kernels' summed time (a rocprofv3
                --kernel-trace --stats run of its own, --merge-stats) plus one empty launch -- the stage adds nodes to
                the graph and nothing else.

  python tools/h2_flow_probe.py --out profiles/h2_flow_probe.json
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o t -- python tools/h2_flow_probe.py --step pipe
  python tools/h2_flow_probe.py --merge-stats DIR/..._kernel_stats.csv --out profiles/h2_flow_probe.json

Without --step this process never opens the GPU: every GPU step is a child process under its own time limit
(timeout -k 10 <s>), the steps are chained and the probe stops at the first one that fails."""
import argparse
import csv
import json
import os
import re
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("k_h2_fc_clear", "k_h2_fc_keys", "k_h2_fc_sums", "k_h2_fc_finish", "k_h2_fc_emit")
STEPS = (("account", 240), ("pipe", 300), ("pipe-base", 300))


def verdicts(res):
    a, p, b = res.get("account"), res.get("pipe"), res.get("pipe-base")
    prof = res.get("profile", {}).get("kernels", {})
    v = {"account_alone": "no expectation set: account_us and empty_launch_us are reported side by side" if isinstance(a, dict) and "account_us" in a
         else "not measured"}
    ok = all(isinstance(x, dict) and "failed" not in x for x in (a, p, b))
    if ok and len(prof) == len(KERNELS):
        base = res.get("parent_ms_per_step", b["ms_per_step"])
        added_us = 1e3 * (p["ms_per_step"] - base)
        bound_us = sum(k["avg_us"] for k in prof.values()) + a["empty_launch_us"]
        v["pipe_step"] = {"added_us": added_us, "bound_us": bound_us, "against": "parent" if "parent_ms_per_step" in res else "same build without ledger",
                          "verdict": "met" if added_us <= bound_us else "missed"}
    else:
        v["pipe_step"] = "not measured"
    res["verdicts"] = v


def merge_stats(path, out):
    res = json.load(open(out)) if os.path.exists(out) else {}
    per = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            for k in KERNELS:
                if re.search(r"\b%s\b" % k, row.get("Name", "")):
                    per[k] = {"calls": int(row["Calls"]), "avg_us": float(row["AverageNs"]) / 1e3}
    res["profile"] = {"kernels": per, "stats_csv": os.path.relpath(path, ROOT)}
    verdicts(res)
    json.dump(res, open(out, "w"), indent=1)
    print(json.dumps(res["profile"]))


def gpu_step(args):
    import torch
    torch.zeros(1, device="cuda")  # (torch's device first: one HIP runtime then serves both)
    torch.cuda.synchronize()
    sys.path.insert(0, ROOT)
    import bench
    import grpc_rdma_amd as g
    from grpc_rdma_amd import h2dev, stream as gs
    g.init(0)
    w = bench.Workload(g, args.msgs)
    ring = args.ring_kb * 1024
    tx, rx = g.Pair(ring, 4095, 0), g.Pair(ring, 4095, 0)
    g.connect_pairs(tx, rx)
    scap = len(w.lens) * 2 + 64 + w.N // 256
    dst_cap = w.N + 16 * scap + 4096
    ev_cap = 4 * len(w.lens) + 1024
    msgs = [(w.payload_buf.ptr + i * w.msg_len, w.msg_len, 1, 0) for i in range(w.n_msgs)]
    keep = []

    def make_job():
        dst = g.DeviceBuffer(nbytes=dst_cap)
        est = max(8, 4 * (w.E // (ring // 2) + 2), 2 * (len(w.lens) // 4095 + 2))
        job = gs.MultiStreamJob([(tx, rx, w.sge, dst.ptr, dst_cap, scap)], est)
        job.set_pipeline(True)
        job.set_sends(2)
        r = job.run(gs.RUN_EAGER)
        job.set_rounds(int(max(-(-int(r.tx_rounds) // 2), r.rx_rounds)))
        r = job.run(gs.RUN_GRAPH)
        assert r.done and r.bytes_delivered == w.N
        keep.extend([dst, job])
        return job, dst

    window = dict(stream_window=(1 << 31) - 1, conn_window=(1 << 31) - 1, conn_threshold=0, max_updates=64)
    if args.step == "account":
        job, dst = make_job()
        p = h2dev.Parser(False)
        assert p.open_streams([1]) == 0
        fc = h2dev.FlowControl(p, **window)
        sl, hdr = g.DeviceBuffer(nbytes=16 * 64), g.DeviceBuffer(nbytes=32 * 64)
        slices = job.delivered_slices(0)
        times = []
        for i in range(2 + 7):
            err, ev = p.deframe(dst.ptr, slices, cap=ev_cap)
            assert err == 0
            _, res, wire = fc.account(sl.ptr, 64, hdr.ptr, 32 * 64)
            assert res[0] == 2 and res[3] == res[4] and len(wire) == 26, res
            if i >= 2:
                times.append(fc.stats()["kernel_us"])
        idle = []
        for i in range(2 + 7):
            p.deframe(dst.ptr, [], cap=ev_cap)
            fc.account(sl.ptr, 64, hdr.ptr, 32 * 64)
            if i >= 2:
                idle.append(fc.stats()["kernel_us"])
        one = torch.zeros(1, dtype=torch.uint8, device="cuda")
        empty = []
        for i in range(10 + 101):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            one.add_(0)
            e1.record()
            e1.synchronize()
            if i >= 10:
                empty.append(1e3 * e0.elapsed_time(e1))
        out = {"events": len(ev), "data_bytes": res[3], "account_us": statistics.median(times), "account_us_all": times,
               "idle_account_us": statistics.median(idle), "empty_launch_us": statistics.median(empty)}
    else:
        with_ledger = args.step == "pipe"
        step_bytes = w.n_msgs * (-(-w.msg_len // 256) * 256)
        pipes = []
        for _ in range(2):
            job, dst = make_job()
            p = h2dev.Parser(False)
            assert p.open_streams([1]) == 0
            pipe = h2dev.Pipe(job, msgs, p, len(job.delivered_slices(0)), ev_cap)
            arena = torch.empty(step_bytes + (4 << 20), dtype=torch.uint8, device="cuda")
            a = h2dev.Assembler(p, arena, 4 << 20, 4096)
            pipe.attach_assembler(a)
            if with_ledger:
                fc = h2dev.FlowControl(p, **window)
                pipe.attach_flow_control(fc)
                keep.append(fc)
            keep.extend([p, arena, a])
            pipes.append(pipe)
        per_round = []
        for rnd in range(args.rounds + 1):
            t0 = time.perf_counter()
            for s in range(args.steps):
                pipes[s % 2].enqueue()
            for pipe in pipes:
                r = pipe.sync()
                assert r["h2_error"] == 0 and r["deframe_overflow"] == 0
            if rnd:  # (round 0 warms up)
                per_round.append(1e3 * (time.perf_counter() - t0) / args.steps)
        out = {"ms_per_step": statistics.median(per_round), "ms_per_step_rounds": per_round, "steps": args.steps}
        if with_ledger:
            _, res, wire = pipes[0].window_updates()
            assert res[0] == 2 and res[7] == 0 and len(wire) == 26, res
            out["frames_per_step"] = res[0]
    print("RESULT " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--msgs", type=int, default=1008)
    ap.add_argument("--ring-kb", type=int, default=256 * 1024)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--step", choices=[s for s, _ in STEPS], default=None, help="one GPU step, in this process")
    ap.add_argument("--parent-ms", type=float, default=None, help="ms per step of --step pipe-base at the parent commit (tools/ab_builds.sh)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--merge-stats", default=None)
    args = ap.parse_args()
    if args.merge_stats:
        merge_stats(args.merge_stats, args.out)
        return
    if args.step:
        gpu_step(args)
        return
    res = {"workload": "%d x 1 MiB messages on stream 1, 16 KiB frames, %d MiB ring, forward pipes with assembler, two "
                       "alternating" % (args.msgs, args.ring_kb >> 10)}
    if args.parent_ms is not None:
        res["parent_ms_per_step"] = args.parent_ms
    for step, limit in STEPS:
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", step, "--msgs", str(args.msgs),
               "--ring-kb", str(args.ring_kb), "--steps", str(args.steps), "--rounds", str(args.rounds)]
        p = subprocess.run(cmd, capture_output=True, text=True)
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not line:
            res[step] = {"failed": p.returncode, "stderr": p.stderr[-500:]}
            print("step %s failed (%d): stopping" % (step, p.returncode))
            break
        res[step] = json.loads(line[-1][7:])
        print(step, json.dumps(res[step]))
    verdicts(res)
    if args.out:
        json.dump(res, open(args.out, "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
