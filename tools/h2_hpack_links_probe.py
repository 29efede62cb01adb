"""The header decoder over a table of links (grdma_h2_hpack_decode_batch) measured against as many single calls
(grdma_h2_hpack_decode) in the same process on the same box.  Medians of --calls repetitions after one warm-up
repetition; the kernel time is the HIP-event time grdma_h2_hpack_stats reports (a batch's: of its six launches; the
singles': the sum over the L calls), the wall time is the host's clock around the call(s).

  The workload is tools/h2_hpack_probe.py's (--requests unary requests of a server connection: the capture's first block,
  then its indexed form, every 16th with a new grpc-timeout; a 64-byte DATA message each), split evenly: for L links each
  link is a connection of its own with requests / L of them.  A repetition uses fresh connections: 2 L parsers with their
  decoders, L for the batch and L twins for the single calls, every one deframed before the clock starts.  Every
  connection is decoded TWICE: the first call of a fresh decoder allocates its scratch tables between the gather and the
  rest; the second call (`*_again_*`: the connection's next requests / L requests, deframed before the clock starts)
  finds them in place and shows the call as a long-lived connection sees it.  (Not where 2 * requests / L is more than
  that workload's generator can put on one connection, about 1 300 requests: no second call at L = 1 with the default.)
  No ratio is fixed in advance: the figures are written down as they come, L = 1 included.

  python tools/h2_hpack_links_probe.py --run --out profiles/h2_hpack_links.json

--legs singles measures the single calls only: that leg uses nothing but grdma_h2_hpack_decode, so the same file put
into a checkout of an earlier commit measures that commit's single call on the same workload.
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def drive(args):
    me = [sys.executable, os.path.abspath(__file__), "--requests", str(args.requests), "--calls", str(args.calls), "--links", args.links,
          "--legs", args.legs]
    cmd = ["timeout", "-k", "10", "420"] + me + (["--out", args.out] if args.out else [])
    rc = subprocess.call(cmd, cwd=ROOT)
    if rc != 0:
        print("step failed with status %d: %s" % (rc, " ".join(cmd)), file=sys.stderr)
    return rc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--requests", type=int, default=1024, help="in all: every link has requests / L of them")
    ap.add_argument("--calls", type=int, default=7, help="repetitions per leg (median)")
    ap.add_argument("--links", default="1,8,64,256")
    ap.add_argument("--legs", default="batch,singles")
    ap.add_argument("--run", action="store_true", help="drive the measuring step as a child process under a time limit")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.run:
        sys.exit(drive(args))
    import torch
    torch.zeros(1, device="cuda")  # (torch's device first: one HIP runtime then serves both)
    torch.cuda.synchronize()
    sys.path.insert(0, ROOT)
    import grpc_rdma_amd as g
    from grpc_rdma_amd import h2dev
    from h2_hpack_probe import workload
    g.init(0)
    legs = args.legs.split(",")
    med = lambda v: statistics.median(v[1:])  # noqa: E731
    rows = []
    for L in [int(x) for x in args.links.split(",")]:
        per = args.requests // L
        wire, blocks, nfields = workload(per)
        try:  # (the same connection going on: its next `per` requests are the second call's)
            both = workload(2 * per)[0]
            assert both.startswith(wire)
            wires = (wire, both[len(wire):])
        except StopIteration:
            # (tools/h2_hpack_probe.py's generator takes a name from the table, and past some 1 300 requests of one
            # connection its grpc-timeout entries have pushed the names out: no second call at that L)
            wires = (wire,)
        # (read only: every link's bytes)
        arenas = [torch.frombuffer(bytearray(w + bytes(64)), dtype=torch.uint8).cuda() for w in wires]
        ev_cap = 16 * per + 1024
        caps = (per + 16, nfields + 64, 1024 * per + 4096)
        targets = [[tuple(g.DeviceBuffer(nbytes=n) for n in (16 * caps[0], 16 * caps[1], caps[2])) for _ in range(L)] for _ in legs]
        t = {leg + again + k: [] for leg in ("batch", "singles") for again in ("", "_again") for k in ("_kernels", "_wall")}
        for _ in range(args.calls + 1):
            sets = []
            for _leg in legs:
                parsers = [h2dev.Parser(True) for _ in range(L)]
                sets.append((parsers, [h2dev.HeaderDecoder(p) for p in parsers]))
            for again, w, arena in zip(("", "_again"), wires, arenas):
                for parsers, _decs in sets:
                    for p in parsers:
                        err, ev = p.deframe(arena.data_ptr(), [(0, len(w))], cap=ev_cap)
                        assert err == 0
                for leg, (parsers, decs), ts in zip(legs, sets, targets):
                    items = [(d, b.ptr, caps[0], f.ptr, caps[1], s.ptr, caps[2]) for d, (b, f, s) in zip(decs, ts)]
                    torch.cuda.synchronize()
                    if leg == "batch":
                        t0 = time.perf_counter()
                        count, res = h2dev.decode_batch(items)
                        t["batch" + again + "_wall"].append(1e6 * (time.perf_counter() - t0))
                        assert count == L, count
                        t["batch" + again + "_kernels"].append(decs[0].stats()["kernel_us"])  # (the batch's, repeated in every item)
                    else:
                        t0 = time.perf_counter()
                        res = [d.decode(*it[1:])[1] for d, it in zip(decs, items)]
                        t["singles" + again + "_wall"].append(1e6 * (time.perf_counter() - t0))
                        t["singles" + again + "_kernels"].append(sum(d.stats()["kernel_us"] for d in decs))
                    assert all((r[0], r[1], r[6], r[7]) == (per, nfields, 0, 0) for r in res), res[:2]
            for parsers, decs in sets:
                for d in decs:
                    d.close()
                for p in parsers:
                    p.close()
        row = {"links": L, "requests_per_link": per, "header_bytes_per_link": sum(len(b) for b in blocks), "fields_per_link": nfields}
        for k, v in t.items():
            if v:
                row[k + "_us"], row[k + "_us_all"] = med(v), v[1:]
        rows.append(row)
        print(json.dumps({k: v for k, v in row.items() if not k.endswith("_all")}), flush=True)
    res = {"workload": "%d unary requests in all, split evenly over the links; a link's connection as tools/h2_hpack_probe.py builds it" % args.requests,
           "calls": args.calls, "legs": legs, "rows": rows}
    print(json.dumps({"done": True, "rows": len(rows)}))
    if args.out:
        json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
