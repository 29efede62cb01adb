"""What a streaming job hands to the HIP runtime -- graph nodes with their dependencies, launches per stream with the
order its events and waits impose, the timed chains -- for every schedule, mode, wire, round count and Sends per plan
of tests/job_schedule_trace.py, against tests/golden/job_schedules.json.  No other CPU test sees a job's ordering (the
emulator runs a graph's nodes in creation order and its streams are synchronous), and on hardware a wrong edge is a
rare wrong byte.

The stored file was written by `python tests/job_schedule_trace.py --golden` from the host layer as it was BEFORE the
schedule table of csrc/grdma_host_job.inc (four hand-written emitters), built with this recorder: it is the reference
the table has to reproduce, exactly.  The one difference the normal form hides on purpose: the in-order timed pass of a
direct wire used to record an event around a wire launch that does not exist (an empty interval the reader skipped)."""
import json
import os

import pytest

from tests import job_schedule_trace as T
from tests.emu_harness import CLANG, emu_lib  # noqa: F401  (emu_lib is a fixture)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "job_schedules.json")


def _golden():
    with open(GOLDEN) as f:
        return json.load(f)


def _deps(line):
    return line.split("<-")[1].split()


def test_the_stored_traces_hold_every_schedule_on_both_wires():
    g = _golden()
    for wire in ("staged", "direct"):
        graphs = {c: g["forms"][p[0][1]].splitlines() for c, p in g["cases"].items() if c.startswith(wire + "/") and p[0][0] == "graph, first run"}
        seq = [c for c, ls in graphs.items() if "/sequential/" in c and all(len(_deps(l)) <= 1 for l in ls[:-1]) and len(ls) >= 9]
        paired = [c for c, ls in graphs.items() if any(l.split()[1] == "k_rx_apply_gather" for l in ls)]
        limit = [c for c, ls in graphs.items() if any(l.split()[1].startswith("k_tx_plan") and len(_deps(l)) > 1 for l in ls)]
        assert seq and paired and limit, (wire, len(seq), len(paired), len(limit))
        assert not set(paired) & set(limit) and not set(seq) & (set(paired) | set(limit))
    hooks = g["forms"][g["cases"]["staged/hooks"][0][1]].splitlines()
    assert hooks[0].split()[1].startswith("k_h2_") and hooks[-1].split()[1].startswith("k_h2_")
    assert any(l.split()[1] == "k_tx_commit" for l in hooks) and _deps(hooks[1]) == ["n0"]


@pytest.mark.skipif(not os.path.exists(CLANG), reason="needs the ROCm clang++ as host compiler")
def test_job_schedules_equal_the_stored_traces(emu_lib, tmp_path):  # noqa: F811
    g = _golden()
    got = T.run_both_wires(str(tmp_path), emu_lib)
    assert sorted(got) == sorted(g["cases"])
    for case, passes in sorted(got.items()):
        want = [[name, g["forms"][i]] for name, i in g["cases"][case]]
        assert [p[0] for p in passes] == [w[0] for w in want], case
        for (name, form), (_, wform) in zip(passes, want):
            assert form == wform, "%s, %s" % (case, name)
