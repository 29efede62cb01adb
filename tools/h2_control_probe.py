"""The control-reply writer (grdma_h2_ctl) measured against its neighbours in the same process on the same box.  HIP
events around the launches, medians of --calls calls after one warm-up call each.

  (a) single   one deframing in the send-window probe's shape (1008 x 1 MiB messages on stream 1, 16 KiB frames) with 64
               PINGs and 2 SETTINGS frames spread through it: grdma_h2_ctl_reply against grdma_h2_sw_intake on the same
               deframing.  Expected: at most 1.5 x the intake's median (both scan the same event list with the same
               grid; the margin covers the extra launches).
  (b) links    32 links, each a deframing of 64 x 64 KiB messages with 8 PINGs: one control_batch against the 32 single
               calls, alternating.  Expected: at most 1.5 x the slowest single call.
  The empty launch: a reply over a deframing without events, a quarter of its four launches.

  python tools/h2_control_probe.py --run --out profiles/h2_control_probe.json

--run is the driver: the measuring step is a child process under a time limit of its own (timeout -k 10 <s> ...), and
the driver stops at a non-zero status.  Without --run the process measures (it needs the device)."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_FRAME = 16384


def drive(args):
    me = [sys.executable, os.path.abspath(__file__), "--msgs", str(args.msgs), "--calls", str(args.calls)]
    cmd = ["timeout", "-k", "10", "420"] + me + (["--out", args.out] if args.out else [])
    rc = subprocess.call(cmd, cwd=ROOT)
    if rc != 0:
        print("step failed with status %d: %s" % (rc, " ".join(cmd)), file=sys.stderr)
    return rc


def frame(ftype, flags, sid, payload=b""):
    return len(payload).to_bytes(3, "big") + bytes([ftype, flags]) + sid.to_bytes(4, "big") + payload


def message_wire(msg_len):
    """one gRPC message of msg_len bytes on stream 1 as DATA frames -> (bytes, [(offset, len)] a header slice and a
    payload slice per frame)"""
    body = bytes([0]) + msg_len.to_bytes(4, "big") + bytes(j * 7 % 251 for j in range(msg_len))
    wire, table = bytearray(), []
    for o in range(0, len(body), MAX_FRAME):
        piece = body[o:o + MAX_FRAME]
        table += [(len(wire), 9), (len(wire) + 9, len(piece))]
        wire += frame(0, 0, 1, piece)
    return bytes(wire), table


def control_frames(n_ping, n_settings):
    out = [frame(6, 0, 0, (0x0102030405060708 + k).to_bytes(8, "big")) for k in range(n_ping)]
    out += [frame(4, 0, 0, (4).to_bytes(2, "big") + (1 << 20).to_bytes(4, "big"))] * n_settings
    return out


def spread(table, n_msgs, per_msg, msg_bytes, ctl, ctl_at):
    """the slice table of n_msgs messages (one message's table repeated) with the control frames, which lie at ctl_at in
    the arena, spread evenly between frames"""
    every = max(1, n_msgs * (per_msg // 2) // (len(ctl) + 1))
    out, k, off, nframes = [], 0, ctl_at, 0
    for m in range(n_msgs):
        for i in range(0, per_msg, 2):
            out += [(table[i][0] + m * msg_bytes, 9), (table[i + 1][0] + m * msg_bytes, table[i + 1][1])]
            nframes += 1
            if nframes % every == 0 and k < len(ctl):
                out.append((off, len(ctl[k])))
                off += len(ctl[k])
                k += 1
    assert k == len(ctl)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--msgs", type=int, default=1008)
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
    g.init(0)
    res = {}

    def arena_of(msg_len, n_msgs, ctl):
        one, table = message_wire(msg_len)
        t = torch.frombuffer(bytearray(one), dtype=torch.uint8).cuda().repeat(n_msgs)
        tail = torch.frombuffer(bytearray(b"".join(ctl) + bytes(64)), dtype=torch.uint8).cuda()
        return torch.cat([t, tail]), spread(table, n_msgs, len(table), len(one), ctl, n_msgs * len(one))

    # ---- (a) one transport --------------------------------------------------------------------------------------------
    arena, table = arena_of(1 << 20, args.msgs, control_frames(64, 2))
    ev_cap = 4 * len(table) + 1024
    parser = h2dev.Parser(False)
    assert parser.open_streams([1]) == 0
    ctl, sw = h2dev.ControlReplies(parser), h2dev.SendWindows(parser)
    sl, hdr = g.DeviceBuffer(nbytes=16 * 64), g.DeviceBuffer(nbytes=32 * 64)
    t_ctl, t_sw = [], []
    for _ in range(args.calls + 1):
        err, ev = parser.deframe(arena.data_ptr(), table, cap=ev_cap)
        assert err == 0
        out = sw.intake()
        assert out[3] == 2 and out[7] == 0
        t_sw.append(sw.stats()["kernel_us"])
        _, r = ctl.reply(sl.ptr, 64, hdr.ptr, 32 * 64)
        assert r[:6] == (66, -(-(64 * 17 + 18) // 23), 64 * 17 + 18, 2, 64, 0), r
        t_ctl.append(ctl.stats()["kernel_us"])
    t_empty = []
    for _ in range(args.calls + 1):
        err, none = parser.deframe(arena.data_ptr(), [], cap=64)
        assert err == 0 and none == []
        sw.intake()
        _, r = ctl.reply(sl.ptr, 64, hdr.ptr, 32 * 64)
        assert r[0] == 0
        t_empty.append(ctl.stats()["kernel_us"])
    empty_launch_us = statistics.median(t_empty[1:]) / 4
    ctl_us, sw_us = statistics.median(t_ctl[1:]), statistics.median(t_sw[1:])
    res["workload"] = "%d x 1 MiB messages on stream 1, 16 KiB frames, 64 PINGs and 2 SETTINGS frames; %d events" % (args.msgs, len(ev))
    res["empty_launch_us"] = empty_launch_us
    res["single"] = {"control_reply_us": ctl_us, "send_window_intake_us": sw_us, "control_reply_us_all": t_ctl[1:],
                     "send_window_intake_us_all": t_sw[1:], "bound_us": 1.5 * sw_us, "verdict": "met" if ctl_us <= 1.5 * sw_us else "missed"}
    ctl.close()
    sw.close()
    parser.close()
    del arena

    # ---- (b) 32 links ---------------------------------------------------------------------------------------------------
    L = 32
    arena, table = arena_of(64 << 10, 64, control_frames(8, 0))
    ev_cap = 4 * len(table) + 1024
    parsers = [h2dev.Parser(False) for _ in range(L)]
    for p in parsers:
        assert p.open_streams([1]) == 0
    ctls = [h2dev.ControlReplies(p) for p in parsers]
    targets = [(g.DeviceBuffer(nbytes=16 * 16), g.DeviceBuffer(nbytes=32 * 16)) for _ in range(L)]

    def deframe_all():
        for p in parsers:
            err, _ = p.deframe(arena.data_ptr(), table, cap=ev_cap)
            assert err == 0

    t_batch, t_slowest, t_sum = [], [], []
    for _ in range(args.calls + 1):
        deframe_all()
        one = []
        for c, (s, h) in zip(ctls, targets):
            _, r = c.reply(s.ptr, 16, h.ptr, 32 * 16)
            assert r[:6] == (8, 6, 136, 0, 8, 0), r
            one.append(c.stats()["kernel_us"])
        t_slowest.append(max(one))
        t_sum.append(sum(one))
        deframe_all()
        out = h2dev.control_batch([(c, s.ptr, 16, h.ptr, 32 * 16) for c, (s, h) in zip(ctls, targets)])
        assert all(r[1][:6] == (8, 6, 136, 0, 8, 0) for r in out)
        t_batch.append(ctls[0].stats()["kernel_us"])
    batch_us, slowest_us = statistics.median(t_batch[1:]), statistics.median(t_slowest[1:])
    res["links"] = {"links": L, "workload": "64 x 64 KiB messages and 8 PINGs a link", "control_batch_us": batch_us,
                    "slowest_single_us": slowest_us, "sum_of_singles_us": statistics.median(t_sum[1:]), "control_batch_us_all": t_batch[1:],
                    "slowest_single_us_all": t_slowest[1:], "bound_us": 1.5 * slowest_us,
                    "verdict": "met" if batch_us <= 1.5 * slowest_us else "missed"}
    print(json.dumps(res))
    if args.out:
        json.dump(res, open(args.out, "w"), indent=1)
    for c in ctls:
        c.close()
    for p in parsers:
        p.close()


if __name__ == "__main__":
    main()
