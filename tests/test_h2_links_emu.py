"""CPU suite for HTTP/2 on many links (k_h2_frame_links, k_h2_deframe_links, the batch entry and the group pipe): its
GPU tests under the wave emulator and the kernels' resources for gfx950."""
import os

import pytest

from tests.emu_harness import CLANG, emu_lib, run_gpu_tests  # noqa: F401  (emu_lib is a fixture)
from tests.kernel_resources import needs_hipcc, report


@pytest.mark.skipif(not os.path.exists(CLANG), reason="needs the ROCm clang++ as host compiler")
def test_links_gpu_tests_under_the_emulator(emu_lib):  # noqa: F811
    # (every test of the file: 3 batch cases, 3 x 2 group-pipe cases, the launch count, the refusals)
    run_gpu_tests(emu_lib, ["tests/test_zz_gpu_h2_links.py", "-n", "4"], 11)


@needs_hipcc
def test_link_kernels_resources():
    """k_h2_frame_links: no scratch, no spills.  k_h2_deframe_links: no more scratch or spills than k_h2_deframe, the
    kernel it shares its body with, in the SAME compile."""
    seen = report("grdma_h2.hip")
    keys = ("scratch", "vspill", "sspill")
    assert {"k_h2_frame_links", "k_h2_deframe_links", "k_h2_deframe"} <= set(seen), sorted(seen)
    assert [seen["k_h2_frame_links"][k] for k in keys] == [0, 0, 0], seen["k_h2_frame_links"]
    for k in keys:
        assert seen["k_h2_deframe_links"][k] <= seen["k_h2_deframe"][k], (k, seen["k_h2_deframe_links"], seen["k_h2_deframe"])
