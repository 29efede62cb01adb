"""The message assembler (grdma_h2_asm) in bench.py's with-h2 shape: the headline workload (1008 x 1 MiB messages on
stream 1, 16 KiB frames), a 256 MiB ring, two alternating pipes over one connection, an arena of more than one step.

Two sets of two pipes over the same connection, one with an assembler attached and one without, are timed in
alternating rounds of --steps steps (each round ends with a sync, so the two sets never overlap).  Reports GiB/s of
user payload for both and checks every message of the last step with torch.equal against the payload.

  python tools/h2_messages_probe.py --out profiles/h2_messages_probe.json
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o t -- python tools/h2_messages_probe.py --with-only
  python tools/h2_messages_probe.py --merge-stats DIR/..._kernel_stats.csv --out profiles/h2_messages_probe.json

--merge-stats adds the plan and copy kernel times of the profiled run to the JSON: copy bandwidth is 2 x payload bytes
per step / copy kernel time, against the 8 TB/s peak."""
import argparse
import csv
import json
import os
import re
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PEAK = 8e12
PLAN = ("k_h2_asm_tiles", "k_h2_asm_carry", "k_h2_asm_begin", "k_h2_asm_bytes", "k_h2_asm_finish")


def merge_stats(path, out):
    res = json.load(open(out)) if os.path.exists(out) else {}
    per = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            name = row.get("Name", "")
            for k in PLAN + ("k_h2_asm_copy", "k_h2_deframe", "k_h2_merge_or_deframe", "k_h2_deframe_chunks"):
                if re.search(r"\b%s\b" % k, name):
                    per[k] = {"calls": int(row["Calls"]), "avg_us": float(row["AverageNs"]) / 1e3}
    plan_us = sum(per[k]["avg_us"] for k in PLAN if k in per)
    copy_us = per.get("k_h2_asm_copy", {}).get("avg_us")
    payload = res.get("payload_bytes_per_step", 1008 << 20)
    kern = {"kernels": per, "plan_us": plan_us, "copy_us": copy_us, "stats_csv": os.path.relpath(path, ROOT)}
    if copy_us:
        kern["copy_frac_of_peak"] = 2 * payload / (copy_us * 1e-6) / PEAK
        kern["plan_over_copy"] = plan_us / copy_us
        kern["targets"] = {"copy >= 0.6 of peak": kern["copy_frac_of_peak"] >= 0.6,
                           "plan <= 10% of copy": kern["plan_over_copy"] <= 0.10}
        if "step_ms_with" in res:
            extra_us = (res["step_ms_with"] - res["step_ms_without"]) * 1e3
            kern["targets"]["with-assembler step slower by <= copy time"] = extra_us <= copy_us
    res["profile"] = kern
    json.dump(res, open(out, "w"), indent=1)
    print(json.dumps(kern))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--msgs", type=int, default=1008)
    ap.add_argument("--ring-kb", type=int, default=256 * 1024)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--with-only", action="store_true", help="only the pipes with the assembler (for the profiled run)")
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
    w = bench.Workload(g, args.msgs)
    ring = args.ring_kb * 1024
    tx, rx = g.Pair(ring, 4095, 0), g.Pair(ring, 4095, 0)
    g.connect_pairs(tx, rx)
    scap = len(w.lens) * 2 + 64 + w.N // 256
    dst_cap = w.N + 16 * scap + 4096
    msgs = [(w.payload_buf.ptr + i * w.msg_len, w.msg_len, 1, 0) for i in range(w.n_msgs)]
    keep = []

    def make_set():
        parser = h2dev.Parser(False)
        assert parser.open_streams([1]) == 0
        pipes = []
        for _ in range(2):
            dst = g.DeviceBuffer(nbytes=dst_cap)
            est = max(8, 4 * (w.E // (ring // 2) + 2), 2 * (len(w.lens) // 4095 + 2))
            job = gs.MultiStreamJob([(tx, rx, w.sge, dst.ptr, dst_cap, scap)], est)
            job.set_pipeline(True)
            job.set_sends(2)
            r = job.run(gs.RUN_EAGER)
            job.set_rounds(int(max(-(-int(r.tx_rounds) // 2), r.rx_rounds)))
            r = job.run(gs.RUN_GRAPH)
            assert r.done and r.bytes_delivered == w.N
            pipes.append(h2dev.Pipe(job, msgs, parser, len(job.delivered_slices(0)), 4 * len(w.lens) + 1024))
            keep.extend([dst, job])
        return parser, pipes

    step_bytes = sum(-(-n // 256) * 256 for n in [w.msg_len] * w.n_msgs)
    arena = torch.empty(step_bytes + (4 << 20), dtype=torch.uint8, device="cuda")
    p_with, pipes_with = make_set()
    asm = h2dev.Assembler(p_with, arena, 4 << 20, 4096)
    for p in pipes_with:
        p.attach_assembler(asm)
    sets = {"with": pipes_with}
    if not args.with_only:
        sets["without"] = make_set()[1]

    def run(pipes, n):
        t0 = time.perf_counter()
        for i in range(n):
            pipes[i % 2].enqueue()
        for p in pipes:
            p.sync()
        return time.perf_counter() - t0

    for name, pipes in sets.items():  # warm-up
        run(pipes, 2)
    times = {k: [] for k in sets}
    for _ in range(args.rounds):
        for name, pipes in sets.items():
            times[name].append(run(pipes, args.steps))
    # the last step of the assembler's set: every message on the device against the payload
    last = pipes_with[(args.steps - 1) % 2]
    r = last.sync()
    got = last.messages()
    refs = [torch.frombuffer(bytearray(m), dtype=torch.uint8).cuda() for m in w.msgs]
    ok = r["h2_error"] == 0 and len(got) == w.n_msgs and all(m.status == 0 and m.length == w.msg_len for m in got)
    ok = ok and all(torch.equal(arena[m.offset:m.offset + m.length], refs[i % len(refs)]) for i, m in enumerate(got))
    payload = w.n_msgs * w.msg_len
    res = {"workload": "%d x %d B messages on stream 1, 16 KiB frames, %d MiB ring, 2 alternating pipes" %
                       (w.n_msgs, w.msg_len, args.ring_kb >> 10),
           "payload_bytes_per_step": payload, "steps_per_round": args.steps, "rounds": args.rounds,
           "last_step_messages_equal": bool(ok), "assembler_stats": asm.stats()}
    for name, ts in times.items():
        ms = 1e3 * min(ts) / args.steps
        res["step_ms_" + name] = ms
        res["gibps_" + name] = payload / (ms * 1e-3) / (1 << 30)
        res["round_s_" + name] = ts
    print(json.dumps(res))
    if args.out:
        old = json.load(open(args.out)) if os.path.exists(args.out) else {}
        old.update(res)
        json.dump(old, open(args.out, "w"), indent=1)
    for p in [q for s in sets.values() for q in s]:
        p.close()
    asm.close()
    if not ok:
        sys.exit(1)


if __name__ == "__main__":
    main()
