"""The message assembler on every link of a multi-connection job (grdma_h2_deframe_messages_batch, the group pipe with
assemblers) in the shape of tools/h2_links_probe.py: 32 links -- 16 pairs, both directions -- of 64 x 64 KiB messages
per link and step, 16 KiB frames, 4 MiB rings, paired schedule, two rounds of slack.

  plan    the five plan kernels of 32 grdma_h2_deframe_messages calls, one per link (Assembler.stats()["plan_us"], HIP
          events): sum, slowest, median -- against the five k_h2_asm_*_links plan kernels of ONE batch call;
  copy    k_h2_asm_copy in one grdma_h2_deframe_messages call on ONE transport that carries the same total (the 32
          links' delivered slices behind one another: the same bytes in the same pieces) against k_h2_asm_copy_links;
  call    wall time around one batch call against the sum of the 32 single calls (median of --calls);
  graph   ms per step of the group pipe with assemblers on all links and without, --rounds regions of --steps steps;
          descriptor count, message bytes and errors checked on every link in the first steps.
  An empty launch is timed between HIP events (grdma_h2_deframe over an empty list).

  python tools/h2_links_messages_probe.py --out profiles/h2_links_messages_probe.json
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o t -- python tools/h2_links_messages_probe.py --profiled
  python tools/h2_links_messages_probe.py --merge-stats DIR/..._kernel_stats.csv --out profiles/h2_links_messages_probe.json

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
PLAN = ("k_h2_asm_tiles", "k_h2_asm_carry", "k_h2_asm_begin", "k_h2_asm_bytes", "k_h2_asm_finish")
KERNELS = tuple(k + s for s in ("_links", "") for k in PLAN + ("k_h2_asm_copy",)) + ("k_h2_deframe_links", "k_h2_deframe")
ALL = 1 << 63
PEAK_BPS = 8e12


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
    if all(k + "_links" in per for k in PLAN + ("k_h2_asm_copy",)):
        six = sum(per[k + "_links"]["avg_us"] for k in PLAN + ("k_h2_asm_copy",))
        prof["six_links_kernels_us"] = round(six, 1)
        prof["plan_links_kernels_us"] = round(sum(per[k + "_links"]["avg_us"] for k in PLAN), 1)
        if "assembly_in_graph_us" in res:
            budget = six + res["empty_launch_us"]
            prof["graph_budget_us"] = round(budget, 1)
            res["expectation_graph_within_six_kernels_plus_empty_launch"] = \
                "met" if res["assembly_in_graph_us"] <= budget else "missed"
    res["profile"] = prof
    json.dump(res, open(out, "w"), indent=1)
    print(json.dumps(res["profile"]))


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
    ap.add_argument("--out", default=None)
    ap.add_argument("--merge-stats", default=None)
    args = ap.parse_args()
    if args.merge_stats:
        merge_stats(args.merge_stats, args.out)
        return
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
    msg_bytes = L * args.msgs * w0.msg_len
    bodies = [w0.msgs[i % len(w0.msgs)] for i in range(args.msgs)]

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

    def parsers(n=L, **kw):
        ps = [h2dev.Parser(False, chunks=False, **kw) for _ in range(n)]
        for p in ps:
            assert p.open_streams([1]) == 0
        return ps

    def assemblers(ps, nbytes=arena_bytes):
        arenas = [g.DeviceBuffer(nbytes=nbytes) for _ in ps]
        return [h2dev.Assembler(p, a, max_pending=max(4096, 2 * L * args.msgs)) for p, a in zip(ps, arenas)], arenas

    def good(err, msgs, asm, n, deep):
        assert err == 0 and len(msgs) == n and all(m.status == 0 and m.length == w0.msg_len for m in msgs), (err, len(msgs))
        if deep:
            assert all(asm.view(m) == bodies[k % args.msgs] for k, m in enumerate(msgs))

    res = {"workload": "%d links (%d pairs, both directions) x %d x %d B messages per step on stream 1, 16 KiB frames, "
                       "%d KiB rings, paired schedule" % (L, L // 2, args.msgs, w0.msg_len, args.ring_kb),
           "message_bytes_per_step": msg_bytes}
    med = statistics.median

    # ---- 32 single calls
    ps_c = parsers()
    as_c, keep_c = assemblers(ps_c)
    plan_rows, copy_rows, wall_c = [], [], []
    for call in range(args.calls + 2):
        prow, crow, wall = [], [], 0.0
        for li in range(L):
            t0 = time.perf_counter()
            err, msgs = ps_c[li].deframe_messages(dsts[li].ptr, delivered[li], as_c[li], ev_cap=ev_cap)
            wall += time.perf_counter() - t0
            good(err, msgs, as_c[li], args.msgs, call == 0)
            st = as_c[li].stats()
            prow.append(st["plan_us"])
            crow.append(st["copy_us"])
            as_c[li].release(ALL)
        plan_rows.append(prow)
        copy_rows.append(crow)
        wall_c.append(wall * 1e6)
    plan_link = [med(r[li] for r in plan_rows[2:]) for li in range(L)]
    copy_link = [med(r[li] for r in copy_rows[2:]) for li in range(L)]
    res["single_calls_plan_us"] = {"sum": sum(plan_link), "slowest": max(plan_link), "median": med(plan_link)}
    res["single_calls_copy_us"] = {"sum": sum(copy_link), "slowest": max(copy_link), "median": med(copy_link)}
    res["single_calls_wall_us_sum"] = round(med(wall_c[2:]), 1)

    # ---- one batch call
    ps_d = parsers()
    as_d, keep_d = assemblers(ps_d)
    items = [(ps_d[li], as_d[li], dsts[li].ptr, delivered[li]) for li in range(L)]
    plan_b, copy_b, wall_b, defr_b = [], [], [], []
    for call in range(args.calls + 2):
        t0 = time.perf_counter()
        got = h2dev.deframe_messages_batch(items, ev_caps=[ev_cap] * L)
        wall_b.append((time.perf_counter() - t0) * 1e6)
        defr_b.append(float(lib.grdma_h2_last_kernel_us()))
        for li, (err, msgs) in enumerate(got):
            good(err, msgs, as_d[li], args.msgs, call == 0)
        st = as_d[0].stats()
        plan_b.append(st["plan_us"])
        copy_b.append(st["copy_us"])
        h2dev.release_batch([(a, ALL) for a in as_d])
    pb, cb, wb, db = med(plan_b[2:]), med(copy_b[2:]), med(wall_b[2:]), med(defr_b[2:])
    res["batch_plan_us"] = pb
    res["batch_copy_us"] = cb
    res["batch_deframe_us"] = round(db, 1)
    res["batch_wall_us"] = round(wb, 1)

    # ---- ONE transport carrying the same total: the links' delivered slices behind one another
    big_host, big_table = bytearray(), []
    for li in range(L):
        base = len(big_host)
        big_host += dsts[li].read(dst_cap)
        big_table += [(base + o, n) for o, n in delivered[li]]
    big_buf = g.DeviceBuffer(data=bytes(big_host))
    del big_host
    p_1 = parsers(1)
    as_1, keep_1 = assemblers(p_1, nbytes=L * arena_bytes)
    copy_1, plan_1 = [], []
    for call in range(args.calls + 2):
        err, msgs = p_1[0].deframe_messages(big_buf.ptr, big_table, as_1[0], ev_cap=L * ev_cap)
        good(err, msgs, as_1[0], L * args.msgs, False)
        st = as_1[0].stats()
        copy_1.append(st["copy_us"])
        plan_1.append(st["plan_us"])
        as_1[0].release(ALL)
    c1 = med(copy_1[2:])
    res["one_transport_same_total"] = {"copy_us": c1, "plan_us": med(plan_1[2:])}
    empty = []
    for _ in range(args.calls + 2):
        p_1[0].deframe(big_buf.ptr, [], cap=64)
        empty.append(float(lib.grdma_h2_last_kernel_us()))
    e_us = med(empty[2:])
    res["empty_launch_us"] = round(e_us, 1)

    # ---- the verdicts (HIP events; the kernel trace's own numbers come with --merge-stats)
    res["plan_batch_over_slowest_single"] = round(pb / max(plan_link), 2)
    res["plan_batch_over_sum_of_singles"] = round(pb / sum(plan_link), 3)
    res["expectation_plan_within_1.5x_slowest_single"] = "met" if pb <= 1.5 * max(plan_link) else "missed"
    res["copy_links_over_one_transport_copy"] = round(cb / c1, 2)
    res["expectation_copy_within_1.25x"] = "met" if cb <= 1.25 * c1 else "missed"
    res["copy_links_fraction_of_8TBps"] = round(2 * msg_bytes / (cb * 1e-6) / PEAK_BPS, 3)
    res["one_transport_copy_fraction_of_8TBps"] = round(2 * msg_bytes / (c1 * 1e-6) / PEAK_BPS, 3)
    res["call_batch_over_sum_of_singles"] = round(wb / med(wall_c[2:]), 3)
    res["call_kernels_plus_empty_launch_us"] = round(db + pb + cb + e_us, 1)
    res["expectation_call_ratio_below_1"] = "met" if wb < med(wall_c[2:]) else "missed"
    res["expectation_call_below_kernels_plus_empty_launch"] = "met" if wb <= db + pb + cb + e_us else "missed"

    # ---- in the graph: the group pipe without, then with assemblers on every link
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

    ps_a = parsers()
    specs = []
    for li, w in enumerate(wls):
        msgs = [(w.payload_buf.ptr + i * w.msg_len, w.msg_len, 1, 0) for i in range(w.n_msgs)]
        specs.append((li, msgs, ps_a[li], len(delivered[li]), ev_cap))
    gp = h2dev.GroupPipe(job, specs)
    ms_without = timed(gp.enqueue, gp.sync)
    as_a, keep_a = assemblers(ps_a)
    gp.attach_assemblers(as_a)
    res["hook_counts_with_assemblers"] = list(gp.hook_counts())
    for step in range(4):
        gp.enqueue()
        r = gp.sync()
        assert all(x["h2_error"] == 0 and x["deframe_overflow"] == 0 and x["frame_overflow"] == 0 for x in r), r
        for li in range(L):
            good(0, gp.messages(li), as_a[li], args.msgs, step == 0 or li in (0, L - 1))
    ms_with = timed(gp.enqueue, gp.sync)
    r = gp.sync()
    assert all(x["h2_error"] == 0 and x["deframe_overflow"] == 0 for x in r)
    good(0, gp.messages(L - 1), as_a[L - 1], args.msgs, True)
    gp.close()
    a, b = med(ms_with), med(ms_without)
    res["group_pipe_ms_per_step"] = {"with_assemblers": ms_with, "without": ms_without}
    res["assembly_in_graph_us"] = round((a - b) * 1e3, 1)
    res["graph_budget_hip_events_us"] = round(pb + cb + e_us, 1)   # (the kernel trace's sum comes with --merge-stats)
    for x in as_a + as_c + as_d + as_1:
        x.close()
    print(json.dumps(res))
    if args.out:
        old = json.load(open(args.out)) if os.path.exists(args.out) else {}
        old.update(res)
        json.dump(old, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
