"""CPU suite for the replies under the peer's windows on many links (k_h2_links_wr_*,
grdma_h2_reply_frame_windowed_batch): its GPU tests under the wave emulator and the link kernels' resources for gfx950
beside their single-transport twins'."""
import os

import pytest

from tests.h2_windowed_reply_lib import HIPCC, STAGES, wr_kernel_resources
from tests.test_emu_gpu_suite import CLANG, emu_lib, run_gpu_tests  # noqa: F401  (emu_lib is a fixture)


@pytest.mark.skipif(not os.path.exists(CLANG), reason="needs the ROCm clang++ as host compiler")
def test_links_windowed_reply_gpu_tests_under_the_emulator(emu_lib):  # noqa: F811
    # (every test of the file, the 256-link case included: nine links over three rounds against single calls, source
    # calls of a batch, trouble that stays with its link, 256 links, the refusals: 5 cases)
    run_gpu_tests(emu_lib, ["tests/test_zz_gpu_h2_links_windowed_reply.py", "-n", "4"], 5)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_link_windowed_reply_kernels_resources(tmp_path):
    """Both many-link kernels exist beside their twins and take no more VGPRs or LDS than the kernel they share their
    source text with, in the same compile."""
    seen = wr_kernel_resources(tmp_path)
    for s in STAGES:
        one, many = seen["k_h2_wr_" + s], seen["k_h2_links_wr_" + s]
        assert (many["scratch"], many["vspill"], many["sspill"]) == (0, 0, 0), (s, many)
        assert many["vgprs"] <= one["vgprs"] and many["lds"] <= one["lds"], (s, one, many)
