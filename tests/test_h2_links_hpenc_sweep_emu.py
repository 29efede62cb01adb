"""CPU suite for the many-link header encoder over the sweep's cases: per family the cases of the by-rule subset
(h2_hpenc_sweep_lib.emu_subset) go through h2dev.encode_batch under the wave emulator, step k of all of them in one call
(tests/h2_links_hpenc_sweep_subset.py, one test per family)."""
import os

import pytest

from tests import h2_hpenc_sweep_lib as L
from tests.emu_harness import CLANG, emu_lib, run_gpu_tests  # noqa: F401  (emu_lib is a fixture)


@pytest.mark.skipif(not os.path.exists(CLANG), reason="needs the ROCm clang++ as host compiler")
def test_links_hpenc_sweep_subset_under_the_emulator(emu_lib):  # noqa: F811
    run_gpu_tests(emu_lib, ["tests/h2_links_hpenc_sweep_subset.py", "-n", "4"], len(L.FAMILIES))
