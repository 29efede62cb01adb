"""CPU suite for the general Send planners over slice lists built from their own edges: every case of the sweep of
tests/test_zz_gpu_send_sweep.py shows its witnesses from the oracle alone (and the restated pricing rule's `sent` equals
the oracle's on every Send of every case: send_sweep_lib.Script asserts it while a case is built), and a by-rule subset
runs under the wave emulator (tests/send_sweep_subset.py, one test per case).  Rule (send_sweep_lib.emu_subset): of
every family the smallest case that asserts more than parity, of the parity-only families I and J the smallest, plus
every case a mutation of profiles/send_sweep.md was caught by alone."""
import collections
import os

import pytest

from tests import send_sweep_lib as L
from tests.emu_harness import CLANG, emu_lib, run_gpu_tests  # noqa: F401  (emu_lib is a fixture)

PER_FAMILY = {"A": 33, "B": 461, "C": 8, "D": 28, "E": 30, "F": 5, "G": 20, "H": 1, "I": 6, "J": 24}


def test_every_case_of_the_send_sweep_shows_its_witnesses():
    cs = L.check_cases()
    assert collections.Counter(c["fam"] for c in cs) == PER_FAMILY
    assert len(cs) == 616 and len(L.tests()) == 1208
    # every Send of every case went through the restatement (Script._one_send asserts sent == the oracle's)
    assert sum(len(L.script_of(c).sends) for c in cs) > 2 * len(cs)
    # what the grid of family B could not build is what the library says, and nothing is marked to be skipped
    assert len(L.B_SKIPPED) == 4 and all(fs == 0 for _p, _m, fs, _v, _b in L.B_SKIPPED)


@pytest.mark.skipif(not os.path.exists(CLANG), reason="needs the ROCm clang++ as host compiler")
def test_send_sweep_subset_under_the_emulator(emu_lib):  # noqa: F811
    subset = L.emu_subset()
    assert len(subset) >= len(L.FAMILIES) == 10 and all(t in subset for t in L.CAUGHT_ALONE)
    run_gpu_tests(emu_lib, ["tests/send_sweep_subset.py", "-n", "4"], len(subset))
