"""CPU suite for the control replies on many links (k_h2_links_ctl_*, grdma_h2_ctl_reply_batch): its GPU tests under the
wave emulator and the kernels' resources for gfx950."""
import os

import pytest

from tests.emu_harness import CLANG, emu_lib, run_gpu_tests  # noqa: F401  (emu_lib is a fixture)
from tests.kernel_resources import kernels_of, needs_hipcc

STAGES = ("last", "mark", "scan", "emit")


@pytest.mark.skipif(not os.path.exists(CLANG), reason="needs the ROCm clang++ as host compiler")
def test_links_control_gpu_tests_under_the_emulator(emu_lib):  # noqa: F811
    # (every test of the file, the 256-link case included: nine links in shuffled order over two calls, batch against
    # single on twin parsers, trouble that stays with its link, 256 links and the refusals: 4 cases)
    run_gpu_tests(emu_lib, ["tests/test_zz_gpu_h2_links_control.py", "-n", "4"], 4)


@needs_hipcc
def test_link_control_kernels_resources():
    """The four many-link kernels exist beside their single-transport twins, none uses scratch or spills, and each takes
    no more VGPRs or LDS than the kernel it shares its source text with, in the same compile."""
    seen = kernels_of("grdma_h2.hip", "k_h2_ctl_", "k_h2_links_ctl_")
    assert set(seen) == {"k_h2_ctl_" + s for s in STAGES} | {"k_h2_links_ctl_" + s for s in STAGES}, sorted(seen)
    for k, v in seen.items():
        assert (v["scratch"], v["vspill"], v["sspill"]) == (0, 0, 0), (k, v)
    for s in STAGES:
        one, many = seen["k_h2_ctl_" + s], seen["k_h2_links_ctl_" + s]
        assert many["vgprs"] <= one["vgprs"] and many["lds"] <= one["lds"], (s, one, many)
