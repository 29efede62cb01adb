"""Send flow control on the device (grdma_h2_sw) in bench.py's with-h2 shape: 1008 x 1 MiB messages on stream 1, 16 KiB
frames.  Two expectations, each measured against its neighbour in the same process on the same box, alternating:

  (a) framing  grdma_h2_sw_frame under open windows against grdma_h2_reply_frame over the descriptors of the same 1008
               messages (the same plan-and-emit structure; the plan adds one keyed scan to the same chain of block
               scans); grdma_h2_frame_messages beside them for scale.  HIP-event time of the launches, median of
               --frames calls each.  Expected: at most the reply framer's median plus one empty launch (half the time of
               grdma_h2_reply_frame over a call without descriptors: its two launches with nothing to do).
  (b) intake   grdma_h2_sw_intake against grdma_h2_fc_account on the same deframing (the 1008 messages' event list), median
               of --frames deframings.  Expected: at most the ledger's median plus one empty launch (fewer stages over
               the same event list).

  python tools/h2_send_window_probe.py --run --out profiles/h2_send_window_probe.json

--run is the driver: the measuring step is a child process under a time limit of its own (timeout -k 10 <s> ...), and
the driver stops at a non-zero status.  Without --run the process measures (it needs the device)."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAXW = (1 << 31) - 1


def drive(args):
    me = [sys.executable, os.path.abspath(__file__), "--msgs", str(args.msgs), "--ring-kb", str(args.ring_kb),
          "--frames", str(args.frames)]
    cmd = ["timeout", "-k", "10", "420"] + me + (["--out", args.out] if args.out else [])
    rc = subprocess.call(cmd, cwd=ROOT)
    if rc != 0:
        print("step failed with status %d: %s" % (rc, " ".join(cmd)), file=sys.stderr)
    return rc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--msgs", type=int, default=1008)
    ap.add_argument("--ring-kb", type=int, default=256 * 1024)
    ap.add_argument("--frames", type=int, default=7, help="calls per leg (median)")
    ap.add_argument("--run", action="store_true", help="drive the measuring step as a child process under a time limit")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.run:
        sys.exit(drive(args))
    import torch
    torch.zeros(1, device="cuda")  # (torch's device first: one HIP runtime then serves both)
    torch.cuda.synchronize()
    sys.path.insert(0, ROOT)
    import bench
    import grpc_rdma_amd as g
    from grpc_rdma_amd import h2dev, stream as gs
    g.init(0)
    lib = g.load()
    w = bench.Workload(g, args.msgs)
    ring = args.ring_kb * 1024
    tx, rx = g.Pair(ring, 4095, 0), g.Pair(ring, 4095, 0)
    g.connect_pairs(tx, rx)
    scap = len(w.lens) * 2 + 64 + w.N // 256
    dst_cap = w.N + 16 * scap + 4096
    ev_cap = 4 * len(w.lens) + 1024
    msgs = [(w.payload_buf.ptr + i * w.msg_len, w.msg_len, 1, 0) for i in range(w.n_msgs)]
    # the forward job once: its delivered slices are the deframing both legs read
    dst = g.DeviceBuffer(nbytes=dst_cap)
    est = max(8, 4 * (w.E // (ring // 2) + 2), 2 * (len(w.lens) // 4095 + 2))
    job = gs.MultiStreamJob([(tx, rx, w.sge, dst.ptr, dst_cap, scap)], est)
    job.set_pipeline(True)
    job.set_sends(2)
    r = job.run(gs.RUN_EAGER)
    job.set_rounds(int(max(-(-int(r.tx_rounds) // 2), r.rx_rounds)))
    r = job.run(gs.RUN_GRAPH)
    assert r.done and r.bytes_delivered == w.N
    delivered = job.delivered_slices(0)
    step_bytes = w.n_msgs * (-(-w.msg_len // 256) * 256)
    res = {"workload": "%d x %d B messages on stream 1, 16 KiB frames" % (w.n_msgs, w.msg_len)}

    parser = h2dev.Parser(False)
    assert parser.open_streams([1]) == 0
    arena = torch.empty(step_bytes + (4 << 20), dtype=torch.uint8, device="cuda")
    asm = h2dev.Assembler(parser, arena, 4 << 20, 4096)
    fc = h2dev.FlowControl(parser, stream_window=MAXW, conn_window=MAXW, conn_threshold=0, max_updates=64)
    sw_rx = h2dev.SendWindows(parser)
    fc_sl, fc_hdr = g.DeviceBuffer(nbytes=16 * 64), g.DeviceBuffer(nbytes=32 * 64)

    # ---- (b) intake against the ledger, on the same deframings ----------------------------------------------------------
    t_fc, t_sw = [], []
    for _ in range(args.frames):
        asm.release(1 << 62)
        err, got = parser.deframe_messages(dst.ptr, delivered, asm, ev_cap=ev_cap, msgs_cap=4096)
        assert err == 0 and len(got) == w.n_msgs
        fc.account(fc_sl.ptr, 64, fc_hdr.ptr, 32 * 64)
        t_fc.append(fc.stats()["kernel_us"])
        out = sw_rx.intake()
        assert out[4] == 0 and out[7] == 0
        t_sw.append(sw_rx.stats()["kernel_us"])

    # ---- (a) framing under open windows against the reply framer over the same messages ---------------------------------
    reply = h2dev.Reply(asm, None, 16384, 4096)
    cap = len(w.lens) + 64
    sl_buf, hdr_buf = g.DeviceBuffer(nbytes=16 * cap), g.DeviceBuffer(nbytes=32 * cap)
    sl_sw, hdr_sw = g.DeviceBuffer(nbytes=16 * cap), g.DeviceBuffer(nbytes=32 * cap)
    p_tx = h2dev.Parser(False)
    assert p_tx.open_streams([1]) == 0
    t_host, t_reply, t_frame = [], [], []
    equal = True
    for _ in range(args.frames):
        n, wire = h2dev.frame_messages(msgs, 16384, sl_buf.ptr, cap, hdr_buf.ptr, 32 * cap)
        t_host.append(float(lib.grdma_h2_last_kernel_us()))
        assert n == len(w.lens) and wire == w.N
        n, st = reply.frame(sl_buf.ptr, cap, hdr_buf.ptr, 32 * cap)
        t_reply.append(st["frame_us"])
        assert n == len(w.lens) and st["wire_bytes"] == w.N
        sw = h2dev.SendWindows(p_tx, MAXW, MAXW, 16384)  # (fresh windows: a call spends them)
        sl, out, prog = sw.frame(msgs, [0] * len(msgs), 16384, sl_sw.ptr, cap, hdr_sw.ptr, 32 * cap)
        t_frame.append(sw.stats()["kernel_us"])
        equal = equal and out[0] == w.n_msgs and out[4] == w.N and [ln for _, ln in sl] == w.lens
        sw.close()
    asm.release(1 << 62)
    empty = g.DeviceBuffer(nbytes=64)
    err, none = parser.deframe_messages(empty.ptr, [], asm, ev_cap=ev_cap, msgs_cap=4096)
    assert err == 0 and none == []
    t_empty = []
    for _ in range(args.frames):
        n0, st = reply.frame(sl_buf.ptr, cap, hdr_buf.ptr, 32 * cap)
        assert n0 == 0
        t_empty.append(st["frame_us"])
    empty_launch_us = statistics.median(t_empty) / 2
    host_us, reply_us, frame_us = (statistics.median(t) for t in (t_host, t_reply, t_frame))
    fc_us, sw_us = statistics.median(t_fc), statistics.median(t_sw)
    res["empty_launch_us"] = empty_launch_us
    res["framing"] = {"send_windows_us": frame_us, "reply_framer_us": reply_us, "host_table_us": host_us,
                      "send_windows_us_all": t_frame, "reply_framer_us_all": t_reply, "slice_table_equal": bool(equal),
                      "bound_us": reply_us + empty_launch_us,
                      "verdict": "met" if frame_us <= reply_us + empty_launch_us else "missed"}
    res["intake"] = {"send_windows_us": sw_us, "ledger_us": fc_us, "send_windows_us_all": t_sw, "ledger_us_all": t_fc,
                     "bound_us": fc_us + empty_launch_us, "verdict": "met" if sw_us <= fc_us + empty_launch_us else "missed"}
    print(json.dumps(res))
    if args.out:
        json.dump(res, open(args.out, "w"), indent=1)
    reply.close()
    fc.close()
    sw_rx.close()
    asm.close()
    if not equal:
        sys.exit(1)


if __name__ == "__main__":
    main()
