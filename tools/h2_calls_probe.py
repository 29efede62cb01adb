"""The call table (grdma_h2_calls) measured on the device.  HIP events around the eight launches of a step (the call's own
stamps), the whole call on the host's clock, medians of --calls steps after one warm-up step.

  unary:   one step for --requests requests on as many streams, one message each, every stream closing in the step
           (reads closed, then left: the table is empty behind it, so the step repeats), over 1, 64 and 4096 registered
           methods
  stream:  a step with no records and 16384 messages on 256 open calls (64 methods)
  copy:    for scale, what a host-side table pays first: the unary step's input tables (blocks, call records, descriptors, events) copied to the host
  Every step's result block is held to the model's (tests/h2_calls_model.py) before its time counts.

  links:   with --links 1,8,64,256: the unary step's calls spread evenly over L links, each with a table of its own; one
           grdma_h2_calls_step_batch against the loop of L single steps in the same run, and one link of 1000 calls
           beside 63 of 4; kernel time and the host's clock as medians with the lowest and the highest

  python tools/h2_calls_probe.py --run --out profiles/h2_calls.json
  python tools/h2_calls_probe.py --run --links 1,8,64,256 --out profiles/h2_calls_links.json

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
    me += ["--links", args.links] if args.links else []
    cmd = ["timeout", "-k", "10", "300"] + me + (["--out", args.out] if args.out else [])
    rc = subprocess.call(cmd, cwd=ROOT)
    if rc != 0:
        print("step failed with status %d: %s" % (rc, " ".join(cmd)), file=sys.stderr)
    return rc


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}


def measure_links(args):
    """the tables of L links: one calls_step_batch against the loop of L single steps, in the same run, turn and turn
    about on twin tables.  The unary step's calls are spread evenly over the links (every link's table is empty behind
    its step, so the step repeats); then one link of 1000 calls beside 63 of 4."""
    sys.path.insert(0, ROOT)
    import grpc_rdma_amd as g
    from grpc_rdma_amd import h2dev
    from tests.h2_calls_lib import Out, Tables
    from tests.h2_calls_model import CallsModel, closed, message, request
    g.init(0)
    n, nm, now = args.requests, 64, 5
    sid = lambda k: 2 * k + 1  # noqa: E731
    res = {"workload": "unary: %d requests over L links (one link of 1000 beside 63 of 4: 1252), one message each, all closing, in one step per "
                       "link; %d methods; the loop of L single steps and one batch step, turn and turn about; medians of %d after a "
                       "warm-up, with the lowest and the highest" % (n, nm, args.calls), "legs": {}}

    def leg(name, sizes):
        links = []
        for c in sizes:
            reqs = [request(sid(k), k % nm, timeout=10**9) for k in range(c)]
            lists = ([r[0] for r in reqs], [r[1] for r in reqs], [message(sid(k), length=100 + k, offset=256 * k) for k in range(c)],
                     [closed(sid(k // 2), k % 2) for k in range(2 * c)])
            want = CallsModel(4096, nm).step(*lists, now, 1 << 30, 1 << 30)[3]  # (the table is empty again behind the step)
            links.append((Tables(g, *lists), want, [(h2dev.CallTable(4096, nm), Out(g, max(1, c), max(1, 2 * c), nm)) for _ in range(2)]))
        items = [(twins[1][0],) + t.args() + (now,) + twins[1][1].args() for t, _, twins in links]
        rows = []
        for _ in range(args.calls + 1):
            t0 = time.perf_counter()
            got = [twins[0][0].step(*t.args(), now, *twins[0][1].args())[1] for t, _, twins in links]
            loop_wall = 1e6 * (time.perf_counter() - t0)
            loop_kernels = sum(twins[0][0].stats()["kernel_us"] for _, _, twins in links)
            t0 = time.perf_counter()
            count, bgot = h2dev.calls_step_batch(items)
            batch_wall = 1e6 * (time.perf_counter() - t0)
            want = [w for _, w, _ in links]
            assert got == want and bgot == want and count == len(links), (name, count)
            rows.append((loop_kernels, loop_wall, links[0][2][1][0].stats()["kernel_us"], batch_wall))
        rows = rows[1:]
        res["legs"][name] = {"links": len(sizes), "calls": sum(sizes), "loop_kernels_us": spread([r[0] for r in rows]),
                             "loop_wall_us": spread([r[1] for r in rows]), "batch_kernels_us": spread([r[2] for r in rows]),
                             "batch_wall_us": spread([r[3] for r in rows]), "all": [list(r) for r in rows]}
        for _, _, twins in links:
            for table, _ in twins:
                table.close()

    for L in [int(x) for x in args.links.split(",")]:
        leg("L%d" % L, [n // L + (1 if k < n % L else 0) for k in range(L)])
    leg("one_of_1000_beside_63_of_4", [1000] + [4] * 63)
    print(json.dumps(res))
    if args.out:
        json.dump(res, open(args.out, "w"), indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--requests", type=int, default=1008)
    ap.add_argument("--calls", type=int, default=7, help="steps per leg (median)")
    ap.add_argument("--links", default=None, help="e.g. 1,8,64,256: measure the batch step over that many links against the loop of single steps")
    ap.add_argument("--run", action="store_true", help="drive the measuring step as a child process under a time limit")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.run:
        sys.exit(drive(args))
    if args.links:
        return measure_links(args)
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
