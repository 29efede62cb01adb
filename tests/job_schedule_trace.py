"""The launch schedule of streaming jobs as the HIP API sees it, reduced to a normal form: the driver behind
tests/test_job_schedule_emu.py.  Run as a script (a child process: the recorder is switched on when the library loads)

    python tests/job_schedule_trace.py OUT.json staged|direct [library]     one wire's cases: {case: [[pass, form], ...]}
    python tests/job_schedule_trace.py --golden OUT.json [library]          both wires, the stored form: golden_of()

against the emulated library (oracle/_build/libgrdma_emu.so), whose HIP stand-in writes one line per launch, graph
node, graph launch, event record and stream wait (tests/cc/hip_api_emu.h, EMU_TRACE_FILE).  Nothing here or in the
recorder knows how the host layer is organised: what is compared is what reaches the runtime.

Normal form of one pass (a string, one item per line):
  graph    `n<i> kernel grid block words <- direct dependencies`, nodes in creation order
  streams  `s<k>: l<i> ...` launches per stream in order, `l<i> kernel grid block words <- predecessors`: the happens-before
           relation (stream order + event waits, transitively closed) written as its transitive reduction, which is
           unique for an order and much shorter
  timed    the launches of the one stream with `E` where events are recorded between them (records without a launch
           between them count once: an empty interval is no interval), and the result's launches_class
Words: `A<k>+off` for a pointer into the k-th allocation the job's trace mentions, integers otherwise; the fourth word
is cut to 32 bits (the planner pair's workgroup split is a 4-byte parameter in an 8-byte slot: the upper half is
padding).  Jobs: one link, 256 KiB ring, max_sge 30."""
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_SO = os.path.join(ROOT, "oracle", "_build", "libgrdma_emu.so")
RING, MAX_SGE = 1 << 18, 30
ROUNDS, SENDS = (1, 2, 3, 5), (1, 2, 8)
# A pipelined job whose drains the steady-state planner keeps declining: after two eager passes grdma_stream_job_run
# has switched rx_fast off, which puts the job on the limit-driven schedule (k_rx_plan behind k_tx_plan_job).  200 slices
# drawn from {100, 257, 513, 700, 3000, 9000} B get there the same way and switch off the same planner (rx_fast), so one
# shape is kept; no shape is known that makes the Sends decline (tx_fast off: k_tx_plan), that choice is not traced.
LIMIT_SLICES = [65536] * 6


class Trace:
    """The recorder's file, read incrementally; names of kernels, allocations, streams and events of one job."""

    def __init__(self, path, lib):
        self.f = open(path, "r")
        self.sym = {}
        for line in subprocess.run(["nm", lib], capture_output=True, text=True, check=True).stdout.splitlines():
            p = line.split()
            if len(p) == 3 and p[1] in "tTwW":
                self.sym.setdefault(int(p[0], 16), p[2])
        self.new_job()

    def new_job(self):
        self.allocs, self.graphs = {}, {}
        self.f.read()

    def kernel(self, rel):
        name = self.sym[int(rel, 16)]
        m = re.match(r"_Z(?:N12_GLOBAL__N_1)?(\d+)", name)   # (a kernel in an unnamed namespace, or a global one)
        return name[m.end():m.end() + int(m.group(1))] if m else name

    def words(self, ws):
        out = []
        for i, w in enumerate(ws):
            if w.startswith("M"):
                base, off = w[1:].split("+")
                out.append("A%d+%s" % (self.allocs.setdefault(base, len(self.allocs)), off))
            else:
                out.append(str(int(w) & 0xFFFFFFFF if i == 3 else int(w)))
        while out and out[-1] == "0":
            out.pop()
        return " ".join(out)

    def take(self):
        """The lines since the last call, graph nodes filed under their graph."""
        ops = []
        for line in self.f.read().splitlines():
            p = line.split()
            if p[0] == "N":
                sep = p.index(":")
                desc = "%s %s %s %s" % (self.kernel(p[2]), ",".join(p[3:6]), ",".join(p[6:9]), self.words(p[9:19]))
                self.graphs.setdefault(p[1], []).append((desc, sorted(int(x) for x in p[sep + 1:])))
            elif p[0] == "L":
                ops.append(("L", "%s %s %s %s" % (self.kernel(p[1]), ",".join(p[2:5]), ",".join(p[5:8]), self.words(p[8:18])), p[18]))
            else:
                ops.append(tuple(p))
        return ops

    def graph_form(self, gid):
        return "\n".join("n%d %s <- %s" % (i, d, " ".join("n%d" % x for x in deps)) for i, (d, deps) in enumerate(self.graphs[gid]))


def streams_form(ops):
    """Launches per stream and the reduced happens-before relation of one pass on streams."""
    streams, launches, before = {}, [], []   # before[i]: set of launches that happen before launch i
    last_on, reach_of_event, pending = {}, {}, {}   # pending[stream]: what the stream's next launch also waits for
    for op in ops:
        if op[0] == "L":
            s, i = op[2], len(launches)
            streams.setdefault(s, []).append(i)
            b = set(pending.get(s, ()))
            if s in last_on:
                b |= before[last_on[s]] | {last_on[s]}
            launches.append(op[1])
            before.append(b)
            last_on[s] = i
        elif op[0] == "R":   # R event stream: the event stands for everything the stream has been given so far
            s = op[2]
            r = set(pending.get(s, ()))
            if s in last_on:
                r |= before[last_on[s]] | {last_on[s]}
            reach_of_event[op[1]] = r
        elif op[0] == "W":   # W stream event
            pending.setdefault(op[1], set()).update(reach_of_event.get(op[2], ()))
            streams.setdefault(op[1], [])
    lines = ["s%d: %s" % (k, " ".join("l%d" % i for i in ls)) for k, ls in enumerate(streams.values()) if ls]
    for i, d in enumerate(launches):
        direct = sorted(x for x in before[i] if not any(x in before[y] for y in before[i]))
        lines.append("l%d %s <- %s" % (i, d, " ".join("l%d" % x for x in direct)))
    return "\n".join(lines)


def timed_form(ops, result):
    out = []
    for op in ops:
        if op[0] == "L":
            out.append(op[1])
        elif op[0] == "R" and (not out or out[-1] != "E"):
            out.append("E")
    assert len({op[2] for op in ops if op[0] == "L"}) == 1, "a timed pass uses one stream"
    return "\n".join(out + ["launches_class " + " ".join(str(int(x)) for x in result.launches_class)])


def main(out_path, wire, lib):
    trace_path = out_path + ".trace"
    open(trace_path, "w").close()
    os.environ["EMU_TRACE_FILE"] = trace_path
    os.environ["GRDMA_LIB_PATH"] = lib
    sys.path.insert(0, ROOT)
    import grpc_rdma_amd as g
    from grpc_rdma_amd import GrdmaError, stream as gs
    g.init(0)
    tr = Trace(trace_path, lib)
    cases = {}

    def keep(case, name, form):
        cases.setdefault(case, []).append([name, form])

    def make_job(lens, flags, rounds):
        bufs = [g.DeviceBuffer(data=bytes((i * 31 + j) % 251 for j in range(min(n, 4096))) * (n // min(n, 4096) + 1))
                for i, n in enumerate(lens)]
        tx, rx = g.Pair(RING, MAX_SGE, flags), g.Pair(RING, MAX_SGE, flags)
        g.connect_pairs(tx, rx)
        total = sum(lens)
        dst_cap = total + 32 * (2 * len(lens) + 64) + 4096
        dst = g.DeviceBuffer(nbytes=dst_cap)
        job = gs.MultiStreamJob([(tx, rx, [(b.ptr, n) for b, n in zip(bufs, lens)], dst.ptr, dst_cap, 2 * len(lens) + 64)], rounds)
        return job, (tx, rx, dst, bufs)

    def graph_pass(case, name, job):
        job.run(gs.RUN_GRAPH)
        ops = tr.take()
        gid = str(int([op for op in ops if op[0] == "X"][-1][1], 16))
        form = tr.graph_form(gid)
        keep(case, name, form)
        return form

    def passes(case, job, schedule, rounds):
        """Every mode of a job, in an order that leaves its planners as they are for as long as possible."""
        f1 = graph_pass(case, "graph, first run", job)
        if rounds == 2:
            graph_pass(case, "graph, index kept", job)
        if schedule == "paired" and rounds >= 2:
            assert "k_rx_apply_gather" in f1, (case, "not the paired schedule")
        if schedule == "limit" and rounds >= 2:
            multi = [l for l in f1.splitlines() if l.split()[1].startswith("k_tx_plan") and len(l.split("<-")[1].split()) > 1]
            assert multi, (case, "not the limit-driven schedule: no send plan with several dependencies")
        try:
            r = job.run(gs.RUN_INSTRUMENTED_SCHEDULE)
            keep(case, "instrumented schedule", timed_form(tr.take(), r))
        except GrdmaError as e:
            tr.take()
            keep(case, "instrumented schedule", "refused: " + str(e))
        r = job.run(gs.RUN_INSTRUMENTED)
        keep(case, "instrumented", timed_form(tr.take(), r))
        job.launch(streams=True)
        job.sync()
        keep(case, "launch_streams", streams_form(tr.take()))
        job.run(gs.RUN_EAGER)
        keep(case, "eager", streams_form(tr.take()))
        if rounds == 2:
            job.set_rebuild_index(True)
            graph_pass(case, "graph, index rebuilt every step", job)

    msgs = []
    from oracle import pyorc
    for i in range(24):
        msgs += pyorc.h2_frame_message(bytes(3000), stream_id=2 * i + 1)[1]
    for flags in ({"staged": 0, "direct": 2}[wire],):
        for rounds in ROUNDS:
            for sends in SENDS:
                variants = [("sequential", {}), ("paired", {})]
                if wire == "staged" and sends != 2:
                    variants += [("paired", {"fused_wire": False}), ("paired", {"promise": True})]
                for schedule, opts in variants:
                    case = "%s/%s%s/r%d/s%d" % (wire, schedule, "".join("+" + k for k in opts), rounds, sends)
                    tr.new_job()
                    job, keepalive = make_job(msgs, flags, rounds)
                    job.set_pipeline(schedule == "paired")
                    if sends > 1:
                        job.set_sends(sends)
                    if "fused_wire" in opts:
                        job.set_fused_wire(False)
                    if "promise" in opts:
                        job.set_promised_credit(True)
                    passes(case, job, schedule, rounds)
                    job.close()
        for rounds in ROUNDS:
            for sends in SENDS:
                case = "%s/limit/r%d/s%d" % (wire, rounds, sends)
                tr.new_job()
                job, keepalive = make_job(LIMIT_SLICES, flags, 6)
                job.set_pipeline(True)
                for _ in range(2):
                    job.run(gs.RUN_EAGER)
                try:
                    job.run(gs.RUN_INSTRUMENTED_SCHEDULE)
                    raise AssertionError((case, "the steady-state planners are still on"))
                except GrdmaError:
                    pass
                tr.take()
                job.set_rounds(rounds)
                if sends > 1:
                    job.set_sends(sends)
                passes(case, job, "limit", rounds)
                job.close()
    if wire == "staged":
        hooks_case(g, gs, tr, keep)
    with open(out_path, "w") as f:
        json.dump(cases, f)
    os.unlink(trace_path)


def hooks_case(g, gs, tr, keep):
    """One fused HTTP/2 pipe step (frame -> job -> deframe inside the job's graph) at the shape of tests/test_gpu_h2.py:
    the pre-hook chain in front of the roots, the post-hook behind k_tx_commit."""
    from grpc_rdma_amd import h2 as h2host, h2dev
    sizes = [70000, 1, 16379, 200000, 16384 * 2 - 5, 5000]
    tr.new_job()
    bufs = [g.DeviceBuffer(data=bytes((j * 7 + i) % 251 for j in range(n))) for i, n in enumerate(sizes)]
    lens = []
    for n in sizes:
        lens += [len(it[1]) if it[0] == "inl" else it[1][1] for it in h2host.frame_message(n, 1, 16384)]
    scratch = g.DeviceBuffer(nbytes=max(lens) + 64)
    tx, rx = g.Pair(RING, MAX_SGE), g.Pair(RING, MAX_SGE)
    g.connect_pairs(tx, rx)
    total = sum(lens)
    scap = 2 * len(lens) + 64 + total // 256
    dst = g.DeviceBuffer(nbytes=total + 16 * scap + 4096)
    job = gs.StreamJob(tx, rx, [(scratch.ptr, n) for n in lens], dst.ptr, total + 16 * scap + 4096, scap, 64)
    r = job.run(gs.RUN_EAGER)
    job.set_rounds(int(max(r.tx_rounds, r.rx_rounds)))
    job.run(gs.RUN_GRAPH)
    parser = h2dev.Parser(False)
    parser.open_streams([1])
    pipe = h2dev.Pipe(job, [(b.ptr, n, 1, 0) for b, n in zip(bufs, sizes)], parser, len(job.delivered_slices(0)), 4 * len(lens) + 256)
    tr.take()
    pipe.enqueue()
    res = pipe.sync()
    assert res["h2_error"] == 0 and res["framed"] == len(lens)
    ops = tr.take()
    keep("staged/hooks", "pipe step", tr.graph_form(str(int([op for op in ops if op[0] == "X"][-1][1], 16))))
    pipe.close()
    job.close()


def run_both_wires(out_dir, lib=EMU_SO):
    """Both wires, one child process each; returns {case: [[pass, form], ...]}."""
    outs = [os.path.join(out_dir, "job_schedules_%s.json" % w) for w in ("staged", "direct")]
    procs = [subprocess.Popen([sys.executable, os.path.abspath(__file__), o, w, lib], cwd=ROOT,
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for o, w in zip(outs, ("staged", "direct"))]
    cases = {}
    for p, o in zip(procs, outs):
        log = p.communicate(timeout=1500)[0]
        assert p.returncode == 0, log[-3000:]
        with open(o) as f:
            cases.update(json.load(f))
    return cases


def golden_of(cases):
    """The stored form: every distinct normal form once, the cases name them by index."""
    forms = {}
    out = {c: [[name, forms.setdefault(form, len(forms))] for name, form in passes] for c, passes in sorted(cases.items())}
    return {"forms": sorted(forms, key=forms.get), "cases": out}


if __name__ == "__main__":
    if sys.argv[1] == "--golden":
        import tempfile
        with tempfile.TemporaryDirectory() as d:
            golden = golden_of(run_both_wires(d, *sys.argv[3:4]))
        with open(sys.argv[2], "w") as f:
            json.dump(golden, f, indent=0, sort_keys=True)
    else:
        main(sys.argv[1], sys.argv[2], sys.argv[3] if len(sys.argv) > 3 else EMU_SO)
