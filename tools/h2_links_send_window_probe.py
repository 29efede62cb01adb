"""Send flow control on many links (grdma_h2_sw_intake_batch, grdma_h2_sw_frame_batch) in the shape of
tools/h2_links_reply_probe.py: 32 links of 64 x 64 KiB messages per link on 64 streams, 16 KiB frames, open windows.

  (a) intake   32 deframings that each carry a WINDOW_UPDATE for the connection and one per stream; 32
               grdma_h2_sw_intake calls, one per link (HIP events: sum, slowest, median), against ONE
               grdma_h2_sw_intake_batch over the same deframings, in alternating rounds of one process.
  (b) framing  32 grdma_h2_sw_frame calls over the links' message tables against ONE grdma_h2_sw_frame_batch over the
               same tables.
  Expectation for both, as for the batched deframer, ledger and reply framer: the batch takes no more than 1.5 x the
  slowest single call -- near one transport's time, not the sum; its ratio to the sum is recorded beside it.
  Medians after two warm-up rounds; the times are the HIP events around the launches (grdma_h2_sw_stats, word 7).

  python tools/h2_links_send_window_probe.py --run --out profiles/h2_links_send_window_probe.json

--run is the driver: each of the two measuring steps is a child process under a time limit of its own (timeout -k 10
<s> ...), one after the other, and the driver stops at the first non-zero status.  A step by hand:

  python tools/h2_links_send_window_probe.py --step intake --out profiles/h2_links_send_window_probe.json

--not-measured writes the JSON with every verdict "not measured" (no MI355X run stands behind the file)."""
import argparse
import json
import os
import statistics
import struct
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VERDICTS = ("expectation_a_intake_batch_within_1.5x_slowest_single", "expectation_b_frame_batch_within_1.5x_slowest_single")
MAXW = (1 << 31) - 1


def workload(args):
    return "%d links x %d x %d B messages per link on %d streams, %d B frames, open windows" % (
        args.links, args.msgs, args.payload, args.msgs, args.max_frame)


def save(out, res):
    if not out:
        return
    old = json.load(open(out)) if os.path.exists(out) else {}
    old.update(res)
    json.dump(old, open(out, "w"), indent=1)


def drive(args):
    """every GPU step a child under its own time limit; the first non-zero status ends the run"""
    me = [sys.executable, os.path.abspath(__file__)]
    shape = ["--links", str(args.links), "--msgs", str(args.msgs), "--payload", str(args.payload), "--max-frame", str(args.max_frame),
             "--calls", str(args.calls)]
    out = args.out or os.path.join(ROOT, "profiles", "h2_links_send_window_probe.json")
    for step in ("intake", "frame"):
        cmd = ["timeout", "-k", "10", "240"] + me + shape + ["--step", step, "--out", out]
        rc = subprocess.call(cmd, cwd=ROOT)
        if rc != 0:
            print("step failed with status %d: %s" % (rc, " ".join(cmd)), file=sys.stderr)
            return rc
    return 0


def verdict(res, key, tag, single, batch):
    med = statistics.median
    b_us = med(batch)
    res["single_calls_%s_us" % tag] = {"sum": round(sum(single), 1), "slowest": round(max(single), 1), "median": round(med(single), 1)}
    res["batch_%s_us" % tag] = round(b_us, 1)
    res["batch_%s_all_us" % tag] = [round(x, 1) for x in batch]
    res["%s_batch_over_slowest_single" % tag] = round(b_us / max(single), 2)
    res["%s_batch_over_sum_of_singles" % tag] = round(b_us / sum(single), 3)
    res[key] = "met" if b_us <= 1.5 * max(single) else "missed"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--links", type=int, default=32)
    ap.add_argument("--msgs", type=int, default=64)
    ap.add_argument("--payload", type=int, default=64 * 1024)
    ap.add_argument("--max-frame", type=int, default=16384)
    ap.add_argument("--calls", type=int, default=9)
    ap.add_argument("--step", choices=("intake", "frame"), default=None)
    ap.add_argument("--run", action="store_true", help="drive both steps as child processes under time limits")
    ap.add_argument("--not-measured", action="store_true", help="write the JSON without a run")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.not_measured:
        res = {"workload": workload(args), "measured_on": "not measured: no MI355X run stands behind this file"}
        res.update({k: "not measured" for k in VERDICTS})
        print(json.dumps(res))
        save(args.out, res)
        return 0
    if args.run:
        return drive(args)
    if not args.step:
        ap.error("one of --run, --step, --not-measured")
    if not os.environ.get("GRDMA_LIB_PATH"):   # (a dry run of the script over the emulated library has no device)
        import torch
        torch.zeros(1, device="cuda")  # (torch's device first: one HIP runtime then serves both)
        torch.cuda.synchronize()
    sys.path.insert(0, ROOT)
    import grpc_rdma_amd as g
    from grpc_rdma_amd import h2dev
    g.init(0)
    L, M = args.links, args.msgs
    ids = [2 * k + 1 for k in range(M)]
    med = statistics.median
    slots = 1
    while slots < 4 * M:
        slots *= 2
    parsers = [h2dev.Parser(False, table_slots=slots, chunks=False) for _ in range(L)]
    for p in parsers:
        assert p.open_streams(ids) == 0
    # (the intake adds credit every round: it starts from RFC 7540's windows; the framer runs under open ones)
    w0 = 65535 if args.step == "intake" else MAXW
    sws = [h2dev.SendWindows(p, w0, w0, (1 << 24) - 1) for p in parsers]
    res = {"workload": workload(args), "measured_on": "one MI355X, HIP events around the launches, medians of %d rounds after 2 warm-up rounds, "
                                                      "single and batch rounds alternating in one process" % args.calls}
    rounds = args.calls + 2

    if args.step == "intake":
        # a WINDOW_UPDATE of 1 for the connection and for every stream: one slice, 13 bytes a frame
        wire = b"".join((4).to_bytes(3, "big") + bytes([8, 0]) + struct.pack(">II", s, 1) for s in [0] + ids)
        assert len(wire) == 13 * (M + 1)
        arena = g.DeviceBuffer(data=wire + bytes(64))
        table = [(0, len(wire))]
        want = (M + 1, 1, M, 0, 0, 0)

        def deframe_all():
            for p in parsers:
                err, ev = p.deframe(arena.ptr, table, cap=8 * (M + 1) + 64)
                assert err == 0, err

        single_rows, batch = [], []
        for r in range(rounds):
            deframe_all()
            row = []
            for s in sws:
                got = s.intake()
                assert got[:6] == want and got[7] == 0, got
                row.append(s.stats()["kernel_us"])
            single_rows.append(row)
            deframe_all()
            got = h2dev.intake_batch(sws)
            assert all(x[:6] == want and x[7] == 0 for x in got), got[0]
            batch.append(sws[0].stats()["kernel_us"])
        single = [med(row[li] for row in single_rows[2:]) for li in range(L)]
        verdict(res, VERDICTS[0], "intake", single, batch[2:])
        res["intake_frames_per_link"] = M + 1
    else:
        pay = g.DeviceBuffer(nbytes=args.payload + 16)
        msgs = [(pay.ptr, args.payload, ids[i], 0) for i in range(M)]
        frames = (5 + args.payload + args.max_frame - 1) // args.max_frame
        cap = 2 * frames * M + 8
        tg = [(g.DeviceBuffer(nbytes=16 * cap), g.DeviceBuffer(nbytes=32 * cap)) for _ in range(L)]
        items = [(sws[li], msgs, [0] * M, args.max_frame, tg[li][0].ptr, cap, tg[li][1].ptr, 32 * cap) for li in range(L)]
        want = (M, 0, 2 * frames * M)
        single_rows, batch, tables = [], [], []
        for r in range(rounds):
            row = []
            for li in range(L):
                sl, got, prog = sws[li].frame(msgs, [0] * M, args.max_frame, tg[li][0].ptr, cap, tg[li][1].ptr, 32 * cap)
                assert got[:3] == want and got[7] == 0 and prog == [5 + args.payload] * M, got
                row.append(sws[li].stats()["kernel_us"])
                if r == 0:
                    tables.append([(p - tg[li][1].ptr if n <= 14 else p, n) for p, n in sl])
            single_rows.append(row)
            out = h2dev.frame_windowed_batch(items)
            assert all(x[1][:3] == want and x[1][7] == 0 for x in out), out[0][1]
            if r == 0:   # the batch's slice tables equal the single calls'
                for li in range(L):
                    assert [(p - tg[li][1].ptr if n <= 14 else p, n) for p, n in out[li][0]] == tables[li], li
            batch.append(sws[0].stats()["kernel_us"])
        single = [med(row[li] for row in single_rows[2:]) for li in range(L)]
        verdict(res, VERDICTS[1], "frame", single, batch[2:])
        res["frame_slices_per_link"] = 2 * frames * M
    for s in sws:
        s.close()
    for p in parsers:
        p.close()
    print(json.dumps(res))
    save(args.out, res)
    return 0


if __name__ == "__main__":
    sys.exit(main())
