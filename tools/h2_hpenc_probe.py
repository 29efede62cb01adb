"""The header encoder (grdma_h2_hpenc) measured on the device.  HIP events around the launches of each stage (the call's
own stamps: scan | walk | emit and commit), the whole call on the host's clock, medians of --calls encoders after one
warm-up encoder.

  The workload: the response headers and the trailers of --replies gRPC replies on as many streams of one connection,
  2 x --replies blocks in one call: HEADERS with :status 200, content-type application/grpc and grpc-accept-encoding,
  then trailers with grpc-status 0 and an empty grpc-message (END_STREAM); every 16th reply fails with a grpc-status
  and a grpc-message of its own.  Every field carries hint 1.
  cold: the first call of a fresh encoder (the table fills); warm: the same call again (almost nothing inserts).
  Beside it: nghttp2's deflater over the same lists, one ctypes call a block, the nva arrays built in front of the
  clock.  That says nothing about a C caller of nghttp2 and is no basis for a claim that the device encoder is ahead of
  a host encoder; it is recorded for scale only, as is the decoder's figure on blocks of this size (profiles/h2_hpack.md).

  python tools/h2_hpenc_probe.py --run --out profiles/h2_hpenc_probe.json

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
    me = [sys.executable, os.path.abspath(__file__), "--replies", str(args.replies), "--calls", str(args.calls)]
    cmd = ["timeout", "-k", "10", "300"] + me + (["--out", args.out] if args.out else [])
    rc = subprocess.call(cmd, cwd=ROOT)
    if rc != 0:
        print("step failed with status %d: %s" % (rc, " ".join(cmd)), file=sys.stderr)
    return rc


def workload(n):
    """-> [(stream, flags, [(name, value, hint)])]: 2 n blocks"""
    lists = []
    for k in range(n):
        sid = 2 * k + 1
        lists.append((sid, 0, [(b":status", b"200", 1), (b"content-type", b"application/grpc", 1),
                               (b"grpc-accept-encoding", b"identity, deflate, gzip", 1)]))
        if k % 16 == 15:
            lists.append((sid, 1, [(b"grpc-status", b"%d" % (1 + k % 13), 1), (b"grpc-message", b"reply %d failed" % k, 1)]))
        else:
            lists.append((sid, 1, [(b"grpc-status", b"0", 1), (b"grpc-message", b"", 1)]))
    return lists


def deflate_all(L, C, lists):
    """nghttp2's deflater over the lists, a call a block -> (seconds cold, seconds warm, bytes cold, bytes warm)"""
    d = L.Deflater()
    prepared = []
    for _, _, hs in lists:
        keep = [(C.create_string_buffer(n, max(1, len(n))), C.create_string_buffer(v, max(1, len(v)))) for n, v, _ in hs]
        nva = (L._NV * len(hs))()
        for i, ((n, v, _), (bn, bv)) in enumerate(zip(hs, keep)):
            nva[i].name, nva[i].value = C.cast(bn, C.POINTER(C.c_uint8)), C.cast(bv, C.POINTER(C.c_uint8))
            nva[i].namelen, nva[i].valuelen, nva[i].flags = len(n), len(v), 0
        prepared.append((keep, nva, len(hs)))
    buf = C.create_string_buffer(4096)
    out = []
    for _ in range(2):
        total = 0
        t0 = time.perf_counter()
        for _, nva, cnt in prepared:
            total += L.NGHTTP2.nghttp2_hd_deflate_hd(d.h, buf, 4096, nva, cnt)
        out.append((time.perf_counter() - t0, total))
    return out[0][0], out[1][0], out[0][1], out[1][1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replies", type=int, default=1008)
    ap.add_argument("--calls", type=int, default=7, help="encoders per leg (median)")
    ap.add_argument("--run", action="store_true", help="drive the measuring step as a child process under a time limit")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.run:
        sys.exit(drive(args))
    import ctypes as C
    sys.path.insert(0, ROOT)
    import grpc_rdma_amd as g
    from grpc_rdma_amd import h2dev
    from tests import h2_hpack_lib as L
    from tests.h2_hpenc_lib import Input
    from tests.h2_hpenc_model import HpencModel, pack
    g.init(0)
    lists = workload(args.replies)
    blocks, fields, arena = pack(lists)
    model = HpencModel()
    expect = [model.encode(blocks, fields, arena, 1 << 30, 1 << 30) for _ in range(2)]  # cold, warm
    inp = Input(g, blocks, fields, arena)
    wire_cap, bw_cap = len(expect[0][0]) + 64, len(blocks) + 16
    wire, bw = g.DeviceBuffer(nbytes=wire_cap), g.DeviceBuffer(nbytes=16 * bw_cap)
    legs = {"cold": [], "warm": []}
    for _ in range(args.calls + 1):  # (a fresh encoder each: the same lists against the same table)
        enc = h2dev.HeaderEncoder()
        for leg, (want, _, res, _) in zip(("cold", "warm"), expect):
            t0 = time.perf_counter()
            n, r = enc.encode(*inp.args(), wire.ptr, wire_cap, bw.ptr, bw_cap)
            wall = 1e6 * (time.perf_counter() - t0)
            assert r == res and wire.read(len(want)) == want, (leg, r, res)
            legs[leg].append(enc.last_stages() + (wall,))
        enc.close()
    med = lambda rows, i: statistics.median(r[i] for r in rows[1:])  # noqa: E731
    res = {"workload": "%d replies: %d blocks, %d fields, %d header-list bytes; wire bytes cold %d, warm %d; inserts cold %d, warm %d" % (
        args.replies, len(blocks), len(fields), len(arena), expect[0][2][2], expect[1][2][2], expect[0][2][3], expect[1][2][3])}
    for leg, rows in legs.items():
        for i, what in enumerate(("scan_us", "walk_us", "emit_commit_us", "kernels_us", "call_wall_us")):
            res["%s_%s" % (leg, what)] = med(rows, i)
        res["%s_all" % leg] = [list(r) for r in rows[1:]]
    if L.NGHTTP2 is not None:
        rows = [deflate_all(L, C, lists) for _ in range(args.calls + 1)][1:]
        res["nghttp2_deflate_ctypes_cold_us"] = 1e6 * statistics.median(r[0] for r in rows)
        res["nghttp2_deflate_ctypes_warm_us"] = 1e6 * statistics.median(r[1] for r in rows)
        res["nghttp2_wire_payload_bytes"] = [rows[0][2], rows[0][3]]
        res["nghttp2_note"] = "one ctypes call a block: says nothing about a C caller"
    print(json.dumps(res))
    if args.out:
        json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
