"""CPU suite for the call table over tables built from its own edges: the witnesses of every case of the sweep
(tests/h2_calls_sweep_lib.py), from the model alone, and the subset small enough for the wave emulator
(tests/h2_calls_sweep_subset.py, one test per case; rule: h2_calls_sweep_lib.emu_subset)."""
import os

import pytest

from tests import h2_calls_sweep_lib as L
from tests.emu_harness import CLANG, emu_lib, run_gpu_tests  # noqa: F401  (emu_lib is a fixture)


def test_every_case_reaches_its_edge():
    L.check_cases()
    assert len(L.CASES) >= 15


@pytest.mark.skipif(not os.path.exists(CLANG), reason="needs the ROCm clang++ as host compiler")
def test_calls_sweep_subset_under_the_emulator(emu_lib):  # noqa: F811
    subset = L.emu_subset()
    assert len(subset) >= 10
    run_gpu_tests(emu_lib, ["tests/h2_calls_sweep_subset.py", "-n", "4"], len(subset))
