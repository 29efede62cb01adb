"""CPU suite for the replies under the peer's windows on many links (k_h2_links_wr_*,
grdma_h2_reply_frame_windowed_batch): its GPU tests under the wave emulator and the link kernels' resources for gfx950
beside their single-transport twins'."""
import os

import pytest

from tests.emu_harness import CLANG, emu_lib, run_gpu_tests  # noqa: F401  (emu_lib is a fixture)
from tests.kernel_resources import kernels_of, needs_hipcc

STAGES = ("queue", "commit")


@pytest.mark.skipif(not os.path.exists(CLANG), reason="needs the ROCm clang++ as host compiler")
def test_links_windowed_reply_gpu_tests_under_the_emulator(emu_lib):  # noqa: F811
    # (every test of the file, the 256-link case included: nine links over three rounds against single calls, source
    # calls of a batch, trouble that stays with its link, 256 links, the refusals: 5 cases)
    run_gpu_tests(emu_lib, ["tests/test_zz_gpu_h2_links_windowed_reply.py", "-n", "4"], 5)


@needs_hipcc
def test_link_windowed_reply_kernels_resources():
    """Both many-link kernels exist beside their twins and take no more VGPRs or LDS than the kernel they share their
    source text with, in the same compile."""
    seen = kernels_of("grdma_h2.hip", "k_h2_wr_", "k_h2_links_wr_")
    for s in STAGES:
        one, many = seen["k_h2_wr_" + s], seen["k_h2_links_wr_" + s]
        assert (many["scratch"], many["vspill"], many["sspill"]) == (0, 0, 0), (s, many)
        assert many["vgprs"] <= one["vgprs"] and many["lds"] <= one["lds"], (s, one, many)
