"""The header encoder over a table of links (grdma_h2_hpenc_encode_batch) measured against as many single calls
(grdma_h2_hpenc_encode) in a loop and against ONE single call for all of it on one link, in the same process on the same
box.  Medians of --calls repetitions after one warm-up repetition; the kernel time is the HIP-event time of the call's
three sections (scan | walk | emit and commit: grdma_h2_hpenc_last_stages; a batch's: of its four launches; the singles':
the sum over the L calls), the wall time is the host's clock around the call(s), which end in a synchronise.

  The workload is tools/h2_hpenc_probe.py's (the response headers and the trailers of --replies gRPC replies, two blocks a
  reply), split evenly: for L links each link is a connection of its own with replies // L of them, its own three input
  tables and its own wire arena.  A repetition uses fresh encoders: L for the batch, L twins for the loop of single calls
  and one for the single call over all L * (replies // L) replies.  Every encoder encodes its input TWICE: `fresh` is the
  first call of a new encoder (the table fills, the scratch tables are allocated), `warm` the same call again (almost
  nothing inserts): the call as a long-lived connection sees it.  Every result tuple is compared with the HpencModel's.
  No ratio is fixed in advance: the figures are written down as they come, L = 1 included.

  python tools/h2_hpenc_links_probe.py --run --out profiles/h2_hpenc_links.json

--legs singles,one measures the single calls only: those legs use nothing but grdma_h2_hpenc_encode, so the same file
put into a checkout of an earlier commit measures that commit's single call on the same workload.
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

SECTIONS = ("scan_us", "walk_us", "emit_commit_us", "kernels_us")


def drive(args):
    me = [sys.executable, os.path.abspath(__file__), "--replies", str(args.replies), "--calls", str(args.calls), "--links", args.links,
          "--legs", args.legs]
    cmd = ["timeout", "-k", "10", "420"] + me + (["--out", args.out] if args.out else [])
    rc = subprocess.call(cmd, cwd=ROOT)
    if rc != 0:
        print("step failed with status %d: %s" % (rc, " ".join(cmd)), file=sys.stderr)
    return rc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replies", type=int, default=1008, help="in all: every link has replies // L of them")
    ap.add_argument("--calls", type=int, default=7, help="repetitions per leg (median)")
    ap.add_argument("--links", default="1,8,64,256")
    ap.add_argument("--legs", default="batch,singles,one")
    ap.add_argument("--run", action="store_true", help="drive the measuring step as a child process under a time limit")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.run:
        sys.exit(drive(args))
    sys.path.insert(0, ROOT)
    import grpc_rdma_amd as g
    from grpc_rdma_amd import h2dev
    from h2_hpenc_probe import workload
    from tests.h2_hpenc_lib import Input
    from tests.h2_hpenc_model import HpencModel, pack
    g.init(0)
    legs = args.legs.split(",")
    med = statistics.median
    rows = []
    for L in [int(x) for x in args.links.split(",")]:
        per = args.replies // L
        lists = workload(per * L)

        def side(tables):
            """a link's input on the device, what the model says of its two calls, its targets"""
            model = HpencModel()
            expect = [model.encode(*tables, 1 << 30, 1 << 30)[2] for _ in range(2)]  # fresh, warm
            wire_cap, bw_cap = expect[0][2] + 64, len(tables[0]) + 16
            return Input(g, *tables), expect, (g.DeviceBuffer(nbytes=wire_cap), wire_cap, g.DeviceBuffer(nbytes=16 * bw_cap), bw_cap)

        links = [side(pack(lists[2 * per * l:2 * per * (l + 1)])) for l in range(L)]  # (two blocks a reply)
        # (the loop's twins read the same inputs and write targets of their own)
        twins = [(inp, exp, (g.DeviceBuffer(nbytes=t[1]), t[1], g.DeviceBuffer(nbytes=16 * t[3]), t[3])) for (inp, exp, t) in links]
        whole = side(pack(lists))

        def args_of(s):
            inp, _exp, (wire, wire_cap, bw, bw_cap) = s
            return inp.args() + (wire.ptr, wire_cap, bw.ptr, bw_cap)

        t = {leg + "_" + state: [] for leg in legs for state in ("fresh", "warm")}
        for _ in range(args.calls + 1):
            for leg in legs:
                n = 1 if leg == "one" else L
                encs = [h2dev.HeaderEncoder() for _ in range(n)]
                for k, state in enumerate(("fresh", "warm")):
                    if leg == "batch":
                        items = [(e,) + args_of(s) for e, s in zip(encs, links)]
                        t0 = time.perf_counter()
                        count, res = h2dev.encode_batch(items)
                        wall = 1e6 * (time.perf_counter() - t0)
                        assert count == L, count
                        stages = encs[0].last_stages()  # (the batch's, repeated in every item)
                        want = [s[1][k] for s in links]
                    elif leg == "singles":
                        calls = [args_of(s) for s in twins]
                        t0 = time.perf_counter()
                        res = [e.encode(*a)[1] for e, a in zip(encs, calls)]
                        wall = 1e6 * (time.perf_counter() - t0)
                        stages = tuple(sum(e.last_stages()[i] for e in encs) for i in range(4))
                        want = [s[1][k] for s in twins]
                    else:
                        a = args_of(whole)
                        t0 = time.perf_counter()
                        res = [encs[0].encode(*a)[1]]
                        wall = 1e6 * (time.perf_counter() - t0)
                        stages = encs[0].last_stages()
                        want = [whole[1][k]]
                    assert res == want, (leg, state, res[:2], want[:2])
                    t[leg + "_" + state].append(tuple(stages) + (wall,))
                for e in encs:
                    e.close()
        row = {"links": L, "replies_per_link": per, "blocks_per_link": 2 * per, "fields_per_link": links[0][0].n[1],
               "wire_bytes_per_link": [links[0][1][0][2], links[0][1][1][2]]}
        for k, v in t.items():
            for i, what in enumerate(SECTIONS + ("wall_us",)):
                row["%s_%s" % (k, what)] = med(r[i] for r in v[1:])
            row[k + "_all"] = [list(r) for r in v[1:]]
        rows.append(row)
        print(json.dumps({k: v for k, v in row.items() if not k.endswith("_all")}), flush=True)
    res = {"workload": "%d replies in all (two blocks each), split evenly over the links; a link's lists as tools/h2_hpenc_probe.py builds them" % args.replies,
           "calls": args.calls, "legs": legs, "rows": rows}
    print(json.dumps({"done": True, "rows": len(rows)}))
    if args.out:
        json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
