"""CPU suite for the header encoder over header lists built from its own edges: a by-rule subset of the sweep of
tests/test_zz_gpu_h2_hpenc_sweep.py runs under the wave emulator (tests/h2_hpenc_sweep_subset.py, one test per case).
Rule (h2_hpenc_sweep_lib.emu_subset): of every family and kind of edge the case with the fewest occurrences, plus every
case a mutation of profiles/h2_hpenc_sweep.md was caught by alone.  The witnesses of all cases, and their calls through the
decoder's model and nghttp2, are in tests/test_h2_hpenc_model.py."""
import os

import pytest

from tests import h2_hpenc_sweep_lib as L
from tests.emu_harness import CLANG, emu_lib, run_gpu_tests  # noqa: F401  (emu_lib is a fixture)


@pytest.mark.skipif(not os.path.exists(CLANG), reason="needs the ROCm clang++ as host compiler")
def test_hpenc_sweep_subset_under_the_emulator(emu_lib):  # noqa: F811
    subset = L.emu_subset()
    assert {L.by_id(cid)["fam"] for cid in subset} == set(L.FAMILIES) and all(cid in subset for cid in L.CAUGHT_ALONE)
    run_gpu_tests(emu_lib, ["tests/h2_hpenc_sweep_subset.py", "-n", "4"], len(subset))
