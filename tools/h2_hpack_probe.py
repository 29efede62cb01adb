"""The header decoder (grdma_h2_hpack) measured against its neighbours in the same process on the same box.  HIP events
around the launches, medians of --calls calls after one warm-up call each.

  The workload: one deframing of --requests unary requests on as many streams of a server connection.  The first block
  is the 234-byte first block of tests/golden/h2_grpcio_capture.json, which fills the dynamic table; the others are its
  fully indexed 9-byte form; every 16th carries a new Huffman-coded grpc-timeout (a literal with incremental indexing and
  an indexed name); each request has one 64-byte DATA message.
  (a) grdma_h2_ctl_reply on the same deframing: it reads the same events and does far less.
  (b) the route a user has without the decoder: the event list and the receive arena copied to the host (timed), then
      the same blocks inflated with nghttp2 on one core (timed apart).  nghttp2 is called through ctypes, one call a
      field; the cost of as many calls of a function that does nothing is measured beside it and reported, not hidden.
  The empty launch: a decode over a deframing without events, a seventh of its seven launches.
  No ratio is fixed in advance: the figures and the verdict "decode <= copy + inflate" are written down as they come.

  python tools/h2_hpack_probe.py --run --out profiles/h2_hpack_probe.json

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
PREFACE = b"PRI * HTTP/2.0\r\n\r\nSM\r\n\r\n"


def drive(args):
    me = [sys.executable, os.path.abspath(__file__), "--requests", str(args.requests), "--calls", str(args.calls)]
    cmd = ["timeout", "-k", "10", "300"] + me + (["--out", args.out] if args.out else [])
    rc = subprocess.call(cmd, cwd=ROOT)
    if rc != 0:
        print("step failed with status %d: %s" % (rc, " ".join(cmd)), file=sys.stderr)
    return rc


def frame(ftype, flags, sid, payload=b""):
    return len(payload).to_bytes(3, "big") + bytes([ftype, flags]) + sid.to_bytes(4, "big") + payload


def workload(n):
    """-> (wire of the connection, [block bytes], fields expected in all)"""
    from tests.h2_hpack_lib import capture_blocks, indexed, literal
    from tests.h2_hpack_model import HpackTable
    first = capture_blocks()[0][1]
    table = HpackTable()
    headers = [(name, value) for name, value, _ in table.decode_block(first)]
    wire, blocks = bytearray(PREFACE + frame(4, 0, 0)), []
    body = bytes([0]) + (64).to_bytes(4, "big") + bytes(range(64))
    for k in range(n):
        if k == 0:
            block = first
        else:
            if k % 16 == 0:
                headers = [(nm, (b"%dm" % (1000 + k)) if nm == b"grpc-timeout" else v) for nm, v in headers]
            out = bytearray()
            for name, value in headers:  # (field by field: an insertion moves the indices of the fields behind it)
                full = [i for i in range(1, 62 + len(table.entries)) if table.get(i) == (name, value)]
                if full:
                    field = indexed(full[0])
                else:
                    named = next(i for i in range(1, 62 + len(table.entries)) if table.get(i)[0] == name)
                    field = literal(named, value, mode=1, hv=True)
                table.decode_block(field)
                out += field
            block = bytes(out)
        blocks.append(block)
        wire += frame(1, 4, 2 * k + 1, block) + frame(0, 1, 2 * k + 1, body)
    return bytes(wire), blocks, len(headers) * n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--requests", type=int, default=1008)
    ap.add_argument("--calls", type=int, default=7, help="calls per leg (median)")
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
    from tests import h2_hpack_lib as L
    g.init(0)
    wire, blocks, nfields = workload(args.requests)
    arena = torch.frombuffer(bytearray(wire + bytes(64)), dtype=torch.uint8).cuda()
    table = [(0, len(wire))]
    ev_cap = 16 * args.requests + 1024
    caps = (args.requests + 16, nfields + 64, 1 << 20)
    t_blocks, t_fields, t_strings = (g.DeviceBuffer(nbytes=16 * caps[0]), g.DeviceBuffer(nbytes=16 * caps[1]), g.DeviceBuffer(nbytes=caps[2]))
    sl, hdr = g.DeviceBuffer(nbytes=16 * 64), g.DeviceBuffer(nbytes=32 * 64)
    t_dec, t_wall, t_ctl, t_empty, nev = [], [], [], [], 0
    for _ in range(args.calls + 1):  # (a fresh connection a call: the same blocks against the same table)
        parser = h2dev.Parser(True)
        dec, ctl = h2dev.HeaderDecoder(parser), h2dev.ControlReplies(parser)
        err, ev = parser.deframe(arena.data_ptr(), table, cap=ev_cap)
        assert err == 0
        nev = len(ev)
        t0 = time.perf_counter()
        n, r = dec.decode(t_blocks.ptr, caps[0], t_fields.ptr, caps[1], t_strings.ptr, caps[2])
        t_wall.append(1e6 * (time.perf_counter() - t0))
        assert (n, r[1], r[6], r[7]) == (args.requests, nfields, 0, 0), r
        t_dec.append(dec.stats()["kernel_us"])
        _, rc = ctl.reply(sl.ptr, 64, hdr.ptr, 32 * 64)
        assert rc[:2] == (1, 1), rc
        t_ctl.append(ctl.stats()["kernel_us"])
        err, none = parser.deframe(arena.data_ptr(), [], cap=64)
        assert err == 0 and none == []
        dec.decode(t_blocks.ptr, caps[0], t_fields.ptr, caps[1], t_strings.ptr, caps[2])
        t_empty.append(dec.stats()["kernel_us"])
        ctl.reply(sl.ptr, 64, hdr.ptr, 32 * 64)
        dec.close()
        ctl.close()
        parser.close()
    # (b) the host route: the copies, then nghttp2 on one core
    events_dev = torch.zeros(24 * nev, dtype=torch.uint8, device="cuda")
    t_copy, t_inflate, t_calls = [], [], []
    for _ in range(args.calls + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        a, e = arena.cpu(), events_dev.cpu()
        t_copy.append(1e6 * (time.perf_counter() - t0))
        if L.NGHTTP2 is not None:
            inf = L.Inflater()
            t0 = time.perf_counter()
            got = sum(len(inf.inflate(b)) for b in blocks)
            t_inflate.append(1e6 * (time.perf_counter() - t0))
            assert got == nfields
            t0 = time.perf_counter()
            for _ in range(nfields + len(blocks)):
                L.NGHTTP2.nghttp2_hd_inflate_get_dynamic_table_size(inf.h)
            t_calls.append(1e6 * (time.perf_counter() - t0))
        del a, e
    med = lambda v: statistics.median(v[1:]) if len(v) > 1 else None  # noqa: E731
    res = {
        "workload": "%d unary requests on %d streams, %d header bytes, %d fields, %d events, %d wire bytes" % (
            args.requests, args.requests, sum(len(b) for b in blocks), nfields, nev, len(wire)),
        "empty_launch_us": med(t_empty) / 7,
        "decode_kernels_us": med(t_dec), "decode_kernels_us_all": t_dec[1:],
        "decode_call_wall_us": med(t_wall), "decode_call_wall_us_all": t_wall[1:],
        "control_reply_us": med(t_ctl), "control_reply_us_all": t_ctl[1:],
        "host_copy_us": med(t_copy), "host_copy_us_all": t_copy[1:],
        "nghttp2_inflate_us": med(t_inflate), "nghttp2_inflate_us_all": t_inflate[1:],
        "ctypes_calls_us": med(t_calls),
    }
    if res["nghttp2_inflate_us"] is not None:
        host = res["host_copy_us"] + res["nghttp2_inflate_us"]
        res["host_route_us"] = host
        res["host_route_without_call_overhead_us"] = res["host_copy_us"] + max(0.0, res["nghttp2_inflate_us"] - res["ctypes_calls_us"])
        res["verdict"] = "decode call (wall) %s copy + inflate" % ("<=" if res["decode_call_wall_us"] <= host else ">")
        res["verdict_without_call_overhead"] = "decode call (wall) %s copy + inflate - ctypes calls" % (
            "<=" if res["decode_call_wall_us"] <= res["host_route_without_call_overhead_us"] else ">")
    print(json.dumps(res))
    if args.out:
        json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
