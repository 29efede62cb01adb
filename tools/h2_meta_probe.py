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

  --links 1,8,64,256 measures the many-link reader instead (CallMetadata.read_batch): the same workload spread evenly
  over L links, one item a link, for every L of the list
  batch:       one read_batch of the L items
  loop:        L single reads of the same items, in the same run, interleaved with the batch
  chain:       at L = 64, h2dev.decode_batch of every link's request headers, read_batch on the decoders' device tables
               (the counts from the decoders' result blocks) and h2dev.encode_batch of the L rejection lists over the
               reader's constant tables; the deframing in front of it is not timed
  uneven:      one link with 1000 blocks beside 63 links of 4: a link's grid is four workgroups whatever it holds

  python tools/h2_meta_probe.py --run --links 1,8,64,256 --out profiles/h2_meta_links.json

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


def spread(n, parts):
    """n requests as evenly as they go over `parts` links -> the number each link takes"""
    return [n // parts + (1 if k < n % parts else 0) for k in range(parts)]


def measure_links(args, g, h2dev):
    """the batch legs -> the result dict"""
    from tests.h2_hpenc_lib import Input
    from tests.h2_hpenc_model import pack
    from tests.h2_meta_model import MetaModel, record_bytes
    methods = [b"/probe.Service/Method%d" % i for i in range(64)]
    lists = workload(args.requests, methods)
    reader = h2dev.CallMetadata(methods=methods)
    med = lambda xs: statistics.median(xs)  # noqa: E731
    res = {"workload": "%d requests of ten fields, every 16th refused, spread evenly over L links; medians of %d after a warm-up" % (args.requests, args.calls)}

    def links_of(parts):
        """parts: the block counts of the links -> per link (Input, record table, rejection list, what the model says)"""
        out, at = [], 0
        for n in parts:
            tables = pack(lists[at:at + n])
            at += n
            recs, rej, want, _ = MetaModel(methods, 1).read(*tables, 1 << 30, 1 << 30)
            out.append((Input(g, *tables), g.DeviceBuffer(nbytes=48 * (n + 1)), g.DeviceBuffer(nbytes=16 * (len(rej) + 1)), (recs, rej, want)))
        return out

    def legs(links):
        """batch and loop, interleaved -> {leg: [(kernels us, wall us)]} without the warm-up"""
        items = [inp.args() + (meta.ptr, len(want[0]) + 1, reject.ptr, len(want[1]) + 1) for inp, meta, reject, want in links]
        rows = {"batch": [], "loop": []}
        for it in range(args.calls + 1):
            t0 = time.perf_counter()
            count, got = reader.read_batch(items)
            wall = 1e6 * (time.perf_counter() - t0)
            rows["batch"].append((reader.stats()["kernel_us"], wall))
            if it == 0:  # the batch wrote what the model says, on every link
                assert count == len(links), count
                for (inp, meta, reject, (recs, rej, want)), r in zip(links, got):
                    assert r == want and meta.read(48 * len(recs)) == b"".join(record_bytes(x) for x in recs), (r, want)
                    assert reject.read(16 * len(rej)) == b"".join(int(w).to_bytes(4, "little") for x in rej for w in x)
            t0 = time.perf_counter()
            for item in items:
                reader.read(*item)
            wall = 1e6 * (time.perf_counter() - t0)
            kernels = 0.0  # (a second pass: reading a call's kernel time is a device read of its own, kept off the clock)
            for item in items:
                reader.read(*item)
                kernels += reader.stats()["kernel_us"]
            rows["loop"].append((kernels, wall))
        return {k: v[1:] for k, v in rows.items()}

    for L in [int(x) for x in args.links.split(",")]:
        rows = legs(links_of(spread(args.requests, L)))
        for leg, r in rows.items():
            res["L%d_%s_kernels_us" % (L, leg)] = med([x[0] for x in r])
            res["L%d_%s_wall_us" % (L, leg)] = med([x[1] for x in r])
            res["L%d_%s_all" % (L, leg)] = [list(x) for x in r]
    # one link of 1000 blocks beside 63 of 4: the big link has its four workgroups and no more
    old, args.requests = lists, 1000 + 63 * 4
    lists = workload(args.requests, methods)
    rows = legs(links_of([4] * 31 + [1000] + [4] * 32))
    rows["big_alone"] = legs(links_of([1000]))["batch"]
    for leg, r in rows.items():
        res["uneven_%s_kernels_us" % leg] = med([x[0] for x in r])
        res["uneven_%s_wall_us" % leg] = med([x[1] for x in r])
        res["uneven_%s_all" % leg] = [list(x) for x in r]
    lists, args.requests = old, len(old)
    res.update(measure_chain(args, g, h2dev, reader, lists, 64))
    reader.close()
    return res


def measure_chain(args, g, h2dev, reader, lists, L):
    """decode batch -> read batch -> encode batch of the refusals on L links -> the result dict's part"""
    from tests.h2_hpack_lib import HH, Targets, headers_frames, literal
    parts, at, per_link = spread(len(lists), L), 0, []
    for n in parts:
        per_link.append(lists[at:at + n])
        at += n
    fp, nf, sp, ns = reader.reject_tables()
    hhs = [HH(g) for _ in range(L)]
    encs = [h2dev.HeaderEncoder() for _ in range(L)]
    targets = [Targets(g, 64, 1024, 1 << 16) for _ in range(L)]
    outs = [(g.DeviceBuffer(nbytes=48 * 65), g.DeviceBuffer(nbytes=16 * 65), g.DeviceBuffer(nbytes=1 << 14), g.DeviceBuffer(nbytes=16 * 65)) for _ in range(L)]
    rows = []
    for it in range(args.calls + 1):
        for hh, mine in zip(hhs, per_link):  # (not timed: the deframing of new streams on every link)
            base = 2 * len(lists) * it
            hh.deframe([b"".join(headers_frames(base + sid, b"".join(literal(n, v, 2) for n, v in hs), flags=1) for sid, _, hs in mine)], checked=False)
        t0 = time.perf_counter()
        _, dres = h2dev.decode_batch([(hh.dec,) + t.args() for hh, t in zip(hhs, targets)])
        t1 = time.perf_counter()
        count, mres = reader.read_batch([(t.blocks.ptr, d[0], t.fields.ptr, d[1], t.strings.ptr, d[2], o[0].ptr, 64, o[1].ptr, 64)
                                         for t, d, o in zip(targets, dres, outs)])
        t2 = time.perf_counter()
        ecount, eres = h2dev.encode_batch([(e, o[1].ptr, m[4], fp, nf, sp, ns, o[2].ptr, 1 << 14, o[3].ptr, 64) for e, m, o in zip(encs, mres, outs)])
        t3 = time.perf_counter()
        assert count == L and ecount == L, (count, ecount)
        assert [m[:2] for m in mres] == [(n, n) for n in parts] and sum(m[4] for m in mres) == len(lists) // 16, mres[:3]
        assert [e[0] for e in eres] == [m[4] for m in mres]
        rows.append([1e6 * (t1 - t0), 1e6 * (t2 - t1), 1e6 * (t3 - t2), 1e6 * (t3 - t0), reader.stats()["kernel_us"]])
    for x in hhs + encs:
        x.close()
    rows = rows[1:]
    keys = ("decode_wall_us", "read_wall_us", "encode_wall_us", "wall_us", "read_kernels_us")
    out = {"chain_L%d_%s" % (L, k): statistics.median(r[i] for r in rows) for i, k in enumerate(keys)}
    out["chain_L%d_all" % L] = rows
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--links", default=None, help="measure the many-link reader over these link counts, e.g. 1,8,64,256")
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
    if args.links:
        res = measure_links(args, g, h2dev)
        print(json.dumps(res))
        if args.out:
            json.dump(res, open(args.out, "w"), indent=1)
        return
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
