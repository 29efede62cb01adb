"""CPU suite for the send-window planner over message tables built from its own edges: every case of the sweep of
tests/test_zz_gpu_h2_send_plan_sweep.py shows its witness from the model alone (tests/h2_send_model.py), and a by-rule
subset runs under the wave emulator (tests/h2_send_plan_sweep_subset.py, one test per case and path).  Rule
(h2_send_plan_sweep_lib.emu_subset): of every family the smallest case on every path it runs on -- family 12, the
intake's grid stride, is hardware only: the emulator's grid is 2 -- plus every test a mutation of
profiles/h2_send_plan_sweep.md was caught by alone."""
import collections
import os

import pytest

from tests import h2_send_plan_sweep_lib as L
from tests.emu_harness import CLANG, emu_lib, run_gpu_tests  # noqa: F401  (emu_lib is a fixture)

PER_FAMILY = {"01": 44, "02": 144, "03": 19, "04": 7, "05": 7, "06": 5, "07": 67, "08": 20, "09": 3, "10": 2, "11": 12, "12": 1}
TESTS_PER_FAMILY = {"01": 45, "02": 145, "03": 33, "04": 7, "05": 8, "06": 6, "07": 75, "08": 21, "09": 6, "10": 3, "11": 12, "12": 1}


def test_every_case_of_the_send_plan_sweep_shows_its_witness():
    cs = L.check_cases()
    assert collections.Counter(c["fam"] for c in cs) == PER_FAMILY
    assert collections.Counter(L.by_id(cid)["fam"] for cid, _ in L.tests()) == TESTS_PER_FAMILY
    assert len(cs) == sum(PER_FAMILY.values()) == 331 and len(L.tests()) == sum(TESTS_PER_FAMILY.values()) == 362
    assert set(PER_FAMILY) == set(L.FAMILIES) and all(c["edge"] for c in cs)


@pytest.mark.skipif(not os.path.exists(CLANG), reason="needs the ROCm clang++ as host compiler")
def test_send_plan_sweep_subset_under_the_emulator(emu_lib):  # noqa: F811
    subset = L.emu_subset()
    fams = {L.by_id(cid)["fam"] for cid, _ in subset}
    assert fams == set(L.FAMILIES) - {"12"} and all(t in subset for t in L.CAUGHT_ALONE)
    run_gpu_tests(emu_lib, ["tests/h2_send_plan_sweep_subset.py", "-n", "4"], len(subset))
