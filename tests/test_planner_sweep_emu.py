"""CPU suite for the stream-job planners over record patterns built from their own edges: a by-rule subset of the sweep of
tests/test_zz_gpu_planner_sweep.py under the wave emulator (tests/planner_sweep_subset.py, one test per case).  Rule
(planner_sweep_lib.emu_subset): of every family the smallest case that asserts more than parity on the schedule whose
bodies the family targets, and family B's F = 193 case on the sequential schedule -- drains in which rxf_body's look-back
step declines.  On the tree before that step had an LDS flag of its own this case aborts here: the emulator finds waves of
one workgroup of k_rx_plan_job at different cross-lane operations, one in the general planner, the others in front of
rxf_body's barrier.  The witnesses of every case of the sweep are checked here too, from the oracle alone (the traces are
kept per process: nothing is computed twice when the GPU module was collected in the same run)."""
import os

import pytest

from tests import planner_sweep_lib as L
from tests.emu_harness import CLANG, emu_lib, run_gpu_tests  # noqa: F401  (emu_lib is a fixture)


def test_every_case_of_the_sweep_shows_its_witnesses():
    n = 0
    for fam in sorted(L.FAMILIES):
        for case in L.cases(fam):
            L.check_witnesses(case)
            n += 1
    assert n == 69


@pytest.mark.skipif(not os.path.exists(CLANG), reason="needs the ROCm clang++ as host compiler")
def test_planner_sweep_subset_under_the_emulator(emu_lib):  # noqa: F811
    subset = L.emu_subset()
    # eleven family lists (A, B, C, D, D2, E, F, G, H, I, J), one case each, and B / F193
    assert len(subset) == 12 and ("B", "F193", "sequential", "staged") in subset
    run_gpu_tests(emu_lib, ["tests/planner_sweep_subset.py", "-n", "4"], len(subset))
