"""CPU suite for send flow control on many links (k_h2_links_sw_*, grdma_h2_sw_intake_batch, grdma_h2_sw_frame_batch):
its GPU tests under the wave emulator and the kernels' resources for gfx950."""
import os

import pytest

from tests.emu_harness import CLANG, emu_lib, run_gpu_tests  # noqa: F401  (emu_lib is a fixture)
from tests.kernel_resources import kernels_of, needs_hipcc

STAGES = ("clear", "take", "finish", "plan", "emit")


@pytest.mark.skipif(not os.path.exists(CLANG), reason="needs the ROCm clang++ as host compiler")
def test_links_send_window_gpu_tests_under_the_emulator(emu_lib):  # noqa: F811
    # (every test of the file, the 256-link case included: it takes a few seconds here.  Intake over nine links, batch
    # against single, trouble, a striding share; framing with resume, emit across links, a cap overflow, the table's
    # limit; the round trip with the ledger; refusals and lifetime: 10 cases)
    run_gpu_tests(emu_lib, ["tests/test_zz_gpu_h2_links_send_window.py", "-n", "4"], 10)


@needs_hipcc
def test_link_send_window_kernels_resources():
    """The five many-link kernels exist beside their single-transport twins, none uses scratch or spills, and clear,
    take, finish and plan take no more VGPRs or LDS than the kernel they share their source text with, in the same
    compile.  (k_h2_links_sw_emit carries the links' prefix in LDS and a search over it: its counts stand in
    docs/h2_deframer.md beside k_h2_sw_emit's and are not bounded by them.)"""
    seen = kernels_of("grdma_h2.hip", "k_h2_sw_", "k_h2_links_sw_")
    assert set(seen) == {"k_h2_sw_" + s for s in STAGES} | {"k_h2_links_sw_" + s for s in STAGES}, sorted(seen)
    for k, v in seen.items():
        assert (v["scratch"], v["vspill"], v["sspill"]) == (0, 0, 0), (k, v)
    for s in STAGES[:4]:
        one, many = seen["k_h2_sw_" + s], seen["k_h2_links_sw_" + s]
        assert many["vgprs"] <= one["vgprs"] and many["lds"] <= one["lds"], (s, one, many)
