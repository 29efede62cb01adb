"""The reply under the peer's windows (grdma_h2_reply_frame_windowed, csrc/grdma_h2_wr.h) measured against its
neighbours in the same process on the same box.  HIP events around the launches, medians of --calls calls after one
warm-up call each.

  (a) single   1008 x 1 MiB descriptors of one standalone call (stream 1, 16 KiB frames), windows open: frame_windowed
               against grdma_h2_sw_frame over the same 1008 messages from a host table.  The new call adds two
               one-workgroup launches that touch about 50 bytes a message.  Expected: at most 1.25 x (that time + two
               empty launches).  grdma_h2_reply_frame over the same descriptors is recorded beside it.
  (b) links    32 links x 64 x 64 KiB messages on 64 streams: one reply_frame_windowed_batch against the 32 single
               calls.  Expected: at most 1.5 x the slowest single call; the sum is recorded.
  (c) a cut    one link of (b) under 65 535-byte stream windows: the call in which every message is cut, and the
               pending_only call behind an intake of the WINDOW_UPDATE frames.  No bound.
  The empty launch: half of grdma_h2_reply_frame over a call without descriptors (its two launches with nothing to do).

  python tools/h2_windowed_reply_probe.py --run --out profiles/h2_windowed_reply_probe.json

--run is the driver: the measuring step is a child process under a time limit of its own (timeout -k 10 <s> ...), and
the driver stops at a non-zero status.  Without --run the process measures (it needs the device)."""
import argparse
import json
import os
import statistics
import struct
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_FRAME = 16384
MAXW = (1 << 31) - 1


def drive(args):
    me = [sys.executable, os.path.abspath(__file__), "--msgs", str(args.msgs), "--calls", str(args.calls)] + \
        (["--no-torch"] if args.no_torch else [])
    cmd = ["timeout", "-k", "10", "420"] + me + (["--out", args.out] if args.out else [])
    rc = subprocess.call(cmd, cwd=ROOT)
    if rc != 0:
        print("step failed with status %d: %s" % (rc, " ".join(cmd)), file=sys.stderr)
    return rc


def frame(ftype, flags, sid, payload=b""):
    return len(payload).to_bytes(3, "big") + bytes([ftype, flags]) + sid.to_bytes(4, "big") + payload


def window_update(sid, inc):
    return frame(8, 0, sid, struct.pack(">I", inc))


def message_wire(msg_len, sid=1):
    """one gRPC message of msg_len bytes on stream sid as DATA frames -> (bytes, [(offset, len)] a header slice and a
    payload slice per frame)"""
    body = bytes([0]) + msg_len.to_bytes(4, "big") + bytes(j * 7 % 251 for j in range(msg_len))
    wire, table = bytearray(), []
    for o in range(0, len(body), MAX_FRAME):
        piece = body[o:o + MAX_FRAME]
        table += [(len(wire), 9), (len(wire) + 9, len(piece))]
        wire += frame(0, 0, sid, piece)
    return bytes(wire), table


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--msgs", type=int, default=1008)
    ap.add_argument("--calls", type=int, default=7, help="calls per leg (median)")
    ap.add_argument("--no-torch", action="store_true", help="arenas from the library's allocator, no torch: a dry run "
                    "under the wave emulator (GRDMA_LIB_PATH) with a small --msgs")
    ap.add_argument("--run", action="store_true", help="drive the measuring step as a child process under a time limit")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.run:
        sys.exit(drive(args))
    if not args.no_torch:
        import torch
        torch.zeros(1, device="cuda")  # (torch's device first: one HIP runtime then serves both)
        torch.cuda.synchronize()
    sys.path.insert(0, ROOT)
    import grpc_rdma_amd as g
    from grpc_rdma_amd import h2dev
    g.init(0)
    res = {}

    class Mem:
        """device memory with .ptr and .nbytes: `data` repeated `times`, or nbytes uninitialised bytes"""

        def __init__(self, data=None, times=1, nbytes=0):
            if args.no_torch:
                self.keep = g.DeviceBuffer(data=data * times) if data is not None else g.DeviceBuffer(nbytes=nbytes)
                self.ptr, self.nbytes = self.keep.ptr, self.keep.nbytes
            else:
                self.keep = (torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda().repeat(times) if data is not None
                             else torch.empty(nbytes, dtype=torch.uint8, device="cuda"))
                self.ptr, self.nbytes = self.keep.data_ptr(), self.keep.numel()

    def credit(parser, sw, frames):
        """WINDOW_UPDATE frames through a plain deframing and the intake"""
        buf = g.DeviceBuffer(data=frames + bytes(64))
        err, _ = parser.deframe(buf.ptr, [(0, len(frames))], cap=4 * len(frames) // 13 + 64)
        assert err == 0
        out = sw.intake()
        assert out[4] == 0 and out[7] == 0, out
        buf.free()

    # ---- (a) one transport, windows open ----------------------------------------------------------------------------------
    n, mlen = args.msgs, 1 << 20
    one, t1 = message_wire(mlen)
    rx = Mem(one, n)
    table = [(o + m * len(one), k) for m in range(n) for o, k in t1]
    ev_cap = 4 * len(table) + 1024
    parser, p_tx = h2dev.Parser(False), h2dev.Parser(False)
    assert parser.open_streams([1]) == 0 and p_tx.open_streams([1]) == 0
    arena = Mem(nbytes=n * mlen + (4 << 20))
    asm = h2dev.Assembler(parser, arena, 4 << 20, 4096)
    sw = h2dev.SendWindows(parser, MAXW, MAXW, MAX_FRAME)
    windowed, plain = h2dev.Reply(asm, None, MAX_FRAME, 4096), h2dev.Reply(asm, None, MAX_FRAME, 4096)
    windowed.attach_windows(sw, 4096)
    cap = len(table) + 64
    sl_a, hdr_a = g.DeviceBuffer(nbytes=16 * cap), g.DeviceBuffer(nbytes=32 * cap)
    sl_b, hdr_b = g.DeviceBuffer(nbytes=16 * cap), g.DeviceBuffer(nbytes=32 * cap)
    t_wr, t_sw, t_plain, equal = [], [], [], True
    for _ in range(args.calls + 1):
        asm.release(1 << 62)
        err, got = parser.deframe_messages(rx.ptr, table, asm, ev_cap=ev_cap, msgs_cap=4096)
        assert err == 0 and len(got) == n
        sw.intake()
        sl_w, st = windowed.frame_windowed(sl_a.ptr, cap, hdr_a.ptr, 32 * cap)
        assert (st["finished"], st["pending"], st["releasable"], st["flags"]) == (n, 0, n, 0), st
        t_wr.append(st["frame_us"])
        k, ps = plain.frame(sl_b.ptr, cap, hdr_b.ptr, 32 * cap)
        t_plain.append(ps["frame_us"])
        msgs = [(arena.ptr + m.offset, m.length, 1, 0) for m in got]
        host = h2dev.SendWindows(p_tx, MAXW, MAXW, MAX_FRAME)  # (fresh windows: a call spends them)
        sl_h, out, prog = host.frame(msgs, [0] * n, MAX_FRAME, sl_b.ptr, cap, hdr_b.ptr, 32 * cap)
        t_sw.append(host.stats()["kernel_us"])
        host.close()
        equal = equal and out[0] == n and out[4] == st["wire_bytes"] and [x for _, x in sl_h] == [x for _, x in sl_w] and k == len(sl_w)
        credit(parser, sw, window_update(0, st["granted"]) + window_update(1, st["granted"]))
    asm.release(1 << 62)
    empty = g.DeviceBuffer(nbytes=64)
    err, none = parser.deframe_messages(empty.ptr, [], asm, ev_cap=ev_cap, msgs_cap=4096)
    assert err == 0 and none == []
    t_empty = []
    for _ in range(args.calls + 1):
        n0, ps = plain.frame(sl_b.ptr, cap, hdr_b.ptr, 32 * cap)
        assert n0 == 0
        t_empty.append(ps["frame_us"])
    empty_launch_us = statistics.median(t_empty[1:]) / 2
    wr_us, sw_us = statistics.median(t_wr[1:]), statistics.median(t_sw[1:])
    bound = 1.25 * (sw_us + 2 * empty_launch_us)
    res["workload"] = "%d x 1 MiB messages on stream 1, 16 KiB frames, windows open" % n
    res["empty_launch_us"] = empty_launch_us
    res["single"] = {"frame_windowed_us": wr_us, "sw_frame_host_table_us": sw_us, "reply_frame_us": statistics.median(t_plain[1:]),
                     "frame_windowed_us_all": t_wr[1:], "sw_frame_host_table_us_all": t_sw[1:], "slice_lists_equal": bool(equal),
                     "bound_us": bound, "verdict": "met" if wr_us <= bound else "missed"}
    for o in (windowed, plain, sw, asm, parser, p_tx):
        o.close()
    del rx, arena

    # ---- (b) 32 links, (c) a window-cut round ----------------------------------------------------------------------------
    L, M, mlen = 32, 64, 64 << 10
    ids = [2 * k + 1 for k in range(M)]
    wires = [message_wire(mlen, s) for s in ids]
    table, off = [], 0
    for w, t in wires:
        table += [(o + off, k) for o, k in t]
        off += len(w)
    rx = Mem(b"".join(w for w, _ in wires) + bytes(64))
    ev_cap = 4 * len(table) + 1024
    cap = len(table) + 64

    class Link:
        def __init__(self, iws):
            self.parser = h2dev.Parser(False)
            assert self.parser.open_streams(ids) == 0
            self.arena = Mem(nbytes=M * mlen + (1 << 20))
            self.asm = h2dev.Assembler(self.parser, self.arena, 4 << 20, 4096)
            self.sw = h2dev.SendWindows(self.parser, iws, MAXW, MAX_FRAME)
            self.reply = h2dev.Reply(self.asm, None, MAX_FRAME, 4096)
            self.reply.attach_windows(self.sw, 4096)
            self.sl, self.hdr = g.DeviceBuffer(nbytes=16 * cap), g.DeviceBuffer(nbytes=32 * cap)

        def receive(self):
            self.asm.release(1 << 62)
            err, got = self.parser.deframe_messages(rx.ptr, table, self.asm, ev_cap=ev_cap, msgs_cap=4096)
            assert err == 0 and len(got) == M
            self.sw.intake()

        def item(self, pending_only=False):
            return (self.reply, self.sl.ptr, cap, self.hdr.ptr, 32 * cap, pending_only)

        def close(self):
            for o in (self.reply, self.sw, self.asm, self.parser):
                o.close()

    links = [Link(MAXW) for _ in range(L)]
    t_batch, t_slowest, t_sum = [], [], []
    for _ in range(args.calls + 1):
        single = []
        for ln in links:
            ln.receive()
            _, st = ln.reply.frame_windowed(*ln.item()[1:5])
            assert (st["finished"], st["pending"]) == (M, 0)
            single.append(st["frame_us"])
        t_slowest.append(max(single))
        t_sum.append(sum(single))
        for ln in links:
            ln.receive()
        out = h2dev.reply_frame_windowed_batch([ln.item() for ln in links])
        assert all(st["finished"] == M and st["overflow"] == 0 for _, st in out)
        t_batch.append(out[0][1]["frame_us"])
    batch_us, slowest_us = statistics.median(t_batch[1:]), statistics.median(t_slowest[1:])
    res["links"] = {"links": L, "workload": "%d x 64 KiB messages on %d streams a link" % (M, M), "batch_us": batch_us,
                    "slowest_single_us": slowest_us, "sum_of_singles_us": statistics.median(t_sum[1:]), "batch_us_all": t_batch[1:],
                    "slowest_single_us_all": t_slowest[1:], "bound_us": 1.5 * slowest_us,
                    "verdict": "met" if batch_us <= 1.5 * slowest_us else "missed"}
    for ln in links:
        ln.close()

    t_cut, t_rest = [], []
    for _ in range(args.calls + 1):
        ln = Link(65535)
        ln.receive()
        _, st = ln.reply.frame_windowed(*ln.item()[1:5])
        assert (st["finished"], st["pending"], st["granted"]) == (0, M, M * 65535), st
        t_cut.append(st["frame_us"])
        credit(ln.parser, ln.sw, b"".join(window_update(s, 100) for s in ids))
        _, st = ln.reply.frame_windowed(*ln.item()[1:5], pending_only=True)
        assert (st["finished"], st["pending"], st["releasable"]) == (M, 0, M), st
        t_rest.append(st["frame_us"])
        ln.close()
    res["cut"] = {"workload": "one link of (b), 65 535-byte stream windows", "every_message_cut_us": statistics.median(t_cut[1:]),
                  "pending_only_behind_an_intake_us": statistics.median(t_rest[1:]), "every_message_cut_us_all": t_cut[1:],
                  "pending_only_behind_an_intake_us_all": t_rest[1:]}
    print(json.dumps(res))
    if args.out:
        json.dump(res, open(args.out, "w"), indent=1)
    if not equal:
        sys.exit(1)


if __name__ == "__main__":
    main()
