"""The call-metadata reader (grdma_h2_meta) measured on the device.  HIP events around the three launches (the call's own
stamps), the whole call on the host's clock, medians of --calls calls after one warm-up call.

  The workload: the request headers of --requests gRPC calls on as many streams of one connection, one block each, in
  one call: the four request pseudo-headers, content-type, te, grpc-timeout, user-agent and two custom fields; 64 paths
  are registered; every 16th request asks for a path nobody registered and is refused.
  read:        CallMetadata.read alone
  read+encode: the read and, behind it on the same stream with no host step in between, HeaderEncoder.encode of the
               rejection list over the reader's constant tables (a fresh encoder per call; its call is synchronous, so
               the wall time is two calls')
  copy:        what the host path pays before it reads a single string: the three tables copied to the host

  python tools/h2_meta_probe.py --run --out profiles/h2_meta.json

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


def workload(n, methods):
    """-> [(stream, flags, [(name, value)])]: n blocks"""
    lists = []
    for k in range(n):
        path = b"/probe.Service/Unknown" if k % 16 == 15 else methods[k % len(methods)]
        lists.append((2 * k + 1, 0, [(b":method", b"POST"), (b":scheme", b"http"), (b":path", path), (b":authority", b"probe.example:50051"),
                                     (b"content-type", b"application/grpc"), (b"te", b"trailers"), (b"grpc-timeout", b"%dm" % (100 + k)),
                                     (b"user-agent", b"grpc-python/1.60.0 grpc-c/37.0.0 (linux; chttp2)"), (b"x-request-id", b"%016x" % (k * 0x9e3779b97f4a7c15 % 2**64)),
                                     (b"x-tenant", b"t%d" % (k % 9))]))
    return lists


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--requests", type=int, default=1008)
    ap.add_argument("--calls", type=int, default=7, help="calls per leg (median)")
    ap.add_argument("--run", action="store_true", help="drive the measuring step as a child process under a time limit")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.run:
        sys.exit(drive(args))
    sys.path.insert(0, ROOT)
    import grpc_rdma_amd as g
    from grpc_rdma_amd import h2dev
    from tests.h2_hpenc_lib import Input
    from tests.h2_hpenc_model import HpencModel, pack
    from tests.h2_meta_model import MetaModel, record_bytes
    g.init(0)
    methods = [b"/probe.Service/Method%d" % i for i in range(64)]
    blocks, fields, arena = pack(workload(args.requests, methods))
    model = MetaModel(methods, 1)
    recs, rej, want, _ = model.read(blocks, fields, arena, 1 << 30, 1 << 30)
    want_meta = b"".join(record_bytes(r) for r in recs)
    want_rej = b"".join(int(w).to_bytes(4, "little") for r in rej for w in r)
    wire_want = HpencModel().encode(rej, model.reject_fields, model.reject_arena, 1 << 30, 1 << 30)
    inp = Input(g, blocks, fields, arena)
    meta, reject = g.DeviceBuffer(nbytes=48 * (len(blocks) + 1)), g.DeviceBuffer(nbytes=16 * (len(rej) + 1))
    wire_cap, bw_cap = len(wire_want[0]) + 64, len(rej) + 16
    wire, bw = g.DeviceBuffer(nbytes=wire_cap), g.DeviceBuffer(nbytes=16 * bw_cap)
    reader = h2dev.CallMetadata(methods=methods)
    fp, nf, sp, ns = reader.reject_tables()
    legs = {"read": [], "read_encode": [], "copy": []}
    for _ in range(args.calls + 1):
        t0 = time.perf_counter()
        n, r = reader.read(*inp.args(), meta.ptr, len(blocks), reject.ptr, len(rej))
        wall = 1e6 * (time.perf_counter() - t0)
        assert r == want and meta.read(len(want_meta)) == want_meta and reject.read(len(want_rej)) == want_rej, (r, want)
        legs["read"].append((reader.stats()["kernel_us"], wall))
        enc = h2dev.HeaderEncoder()
        t0 = time.perf_counter()
        n, r = reader.read(*inp.args(), meta.ptr, len(blocks), reject.ptr, len(rej))
        nfr, er = enc.encode(reject.ptr, n, fp, nf, sp, ns, wire.ptr, wire_cap, bw.ptr, bw_cap)
        wall = 1e6 * (time.perf_counter() - t0)
        assert er == wire_want[2] and wire.read(len(wire_want[0])) == wire_want[0], (er, wire_want[2])
        legs["read_encode"].append((reader.stats()["kernel_us"] + enc.last_stages()[3], wall))  # (both kept on the host)
        enc.close()
        t0 = time.perf_counter()
        inp.blocks.read(16 * len(blocks)), inp.fields.read(16 * len(fields)), inp.strings.read(len(arena))
        legs["copy"].append((0.0, 1e6 * (time.perf_counter() - t0)))
    reader.close()
    med = lambda rows, i: statistics.median(r[i] for r in rows[1:])  # noqa: E731
    res = {"workload": "%d requests: %d blocks, %d fields, %d string bytes; %d refused, %d wire bytes of Trailers-Only responses" % (
        args.requests, len(blocks), len(fields), len(arena), len(rej), len(wire_want[0]))}
    for leg, rows in legs.items():
        if leg != "copy":
            res["%s_kernels_us" % leg] = med(rows, 0)
        res["%s_wall_us" % leg] = med(rows, 1)
        res["%s_all" % leg] = [list(r) for r in rows[1:]]
    print(json.dumps(res))
    if args.out:
        json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
