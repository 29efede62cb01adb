"""The call table (grdma_h2_calls) measured on the device.  HIP events around the eight launches of a step (the call's own
stamps), the whole call on the host's clock, medians of --calls steps after one warm-up step.

  unary:   one step for --requests requests on as many streams, one message each, every stream closing in the step
           (reads closed, then left: the table is empty behind it, so the step repeats), over 1, 64 and 4096 registered
           methods
  stream:  a step with no records and 16384 messages on 256 open calls (64 methods)
  copy:    for scale, what a host-side table pays first: the unary step's input tables (blocks, call records, descriptors, events) copied to the host
  Every step's result block is held to the model's (tests/h2_calls_model.py) before its time counts.

  python tools/h2_calls_probe.py --run --out profiles/h2_calls.json

--run is the driver: the measuring step is a child process under a time limit of its own (timeout -k 10 <s> ...), and
the driver stops at a non-zero status.  Without --run the process measures (it needs the device)."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def drive(args):
    me = [sys.executable, os.path.abspath(__file__), "--requests", str(args.requests), "--calls", str(args.calls)]
    cmd = ["timeout", "-k", "10", "300"] + me + (["--out", args.out] if args.out else [])
    rc = subprocess.call(cmd, cwd=ROOT)
    if rc != 0:
        print("step failed with status %d: %s" % (rc, " ".join(cmd)), file=sys.stderr)
    return rc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--requests", type=int, default=1008)
    ap.add_argument("--calls", type=int, default=7, help="steps per leg (median)")
    ap.add_argument("--run", action="store_true", help="drive the measuring step as a child process under a time limit")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.run:
        sys.exit(drive(args))
    sys.path.insert(0, ROOT)
    import grpc_rdma_amd as g
    from grpc_rdma_amd import h2dev
    from tests.h2_calls_lib import Out, Tables
    from tests.h2_calls_model import CallsModel, closed, message, request
    g.init(0)
    n = args.requests
    res = {"workload": "unary: %d requests, one message each, all closing, in one step; stream: 16384 messages on 256 open calls; "
                       "medians of %d after a warm-up" % (n, args.calls)}

    def leg(name, table, model, tables, lists, out, now):
        rows = []
        for _ in range(args.calls + 1):
            want = model.step(*lists, now, 1 << 30, 1 << 30)[3]
            t0 = time.perf_counter()
            _, got = table.step(*tables.args(), now, *out.args())
            wall = 1e6 * (time.perf_counter() - t0)
            assert got == want, (got, want)
            rows.append((table.stats()["kernel_us"], wall))
        res["%s_kernels_us" % name] = statistics.median(r[0] for r in rows[1:])
        res["%s_wall_us" % name] = statistics.median(r[1] for r in rows[1:])
        res["%s_all" % name] = [list(r) for r in rows[1:]]

    sid = lambda k: 2 * k + 1  # noqa: E731
    for nm in (1, 64, 4096):
        reqs = [request(sid(k), k % nm, timeout=10**9) for k in range(n)]
        lists = ([r[0] for r in reqs], [r[1] for r in reqs], [message(sid(k), length=100 + k, offset=256 * k) for k in range(n)],
                 [closed(sid(k // 2), k % 2) for k in range(2 * n)])
        tables, out = Tables(g, *lists), Out(g, n, 2 * n, nm)
        table = h2dev.CallTable(4096, nm)
        leg("unary_m%d" % nm, table, CallsModel(4096, nm), tables, lists, out, 5)
        if nm == 64:
            rows = []
            for _ in range(args.calls + 1):
                t0 = time.perf_counter()
                tables.blocks.read(16 * n), tables.meta.read(48 * n), tables.msgs.read(40 * n), tables.events.read(24 * 2 * n)
                rows.append(1e6 * (time.perf_counter() - t0))
            res["copy_wall_us"] = statistics.median(rows[1:])
            res["copy_all"] = rows[1:]
        table.close()
    table, model = h2dev.CallTable(4096, 64), CallsModel(4096, 64)
    reqs = [request(sid(k), k % 64) for k in range(256)]
    opening = ([r[0] for r in reqs], [r[1] for r in reqs], [], [])
    model.step(*opening, 0, 1 << 30, 1 << 30)
    t0, o0 = Tables(g, *opening), Out(g, 1, 1, 64)
    table.step(*t0.args(), 0, *o0.args())
    lists = ([], [], [message(sid(i * 37 % 256), length=i % 999, offset=256 * i) for i in range(16384)], [])
    leg("stream", table, model, Tables(g, *lists), lists, Out(g, 16384, 1, 64), 1)
    table.close()
    print(json.dumps(res))
    if args.out:
        json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
