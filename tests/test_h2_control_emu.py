"""CPU suite for the control replies on the device (SETTINGS ACK, PING ACK, RST_STREAM: k_h2_ctl_*, grdma_h2_ctl_*): its
GPU tests under the wave emulator and the kernels' resources for gfx950."""
import os

import pytest

from tests.emu_harness import CLANG, emu_lib, run_gpu_tests  # noqa: F401  (emu_lib is a fixture)
from tests.kernel_resources import kernels_of, needs_hipcc

KERNELS = ("k_h2_ctl_last", "k_h2_ctl_mark", "k_h2_ctl_scan", "k_h2_ctl_emit")


@pytest.mark.skipif(not os.path.exists(CLANG), reason="needs the ROCm clang++ as host compiler")
def test_control_gpu_tests_under_the_emulator(emu_lib):  # noqa: F811
    # (every test of the file: whole frames, 1-byte slices, the capture, PING, SETTINGS and GOAWAY cut between calls,
    # what the peer acknowledged, two GOAWAYs, order, replies spanning both workgroups of the emulator's grid, no control
    # frame, a connection error, lost calls, cap overflows and their repeat, ledger and send windows beside the writer,
    # refusals and lifetime: 30 cases)
    run_gpu_tests(emu_lib, ["tests/test_zz_gpu_h2_control.py", "-n", "4"], 30)


@needs_hipcc
def test_control_kernels_resources():
    """The four kernels exist and use no scratch and spill nothing."""
    seen = kernels_of("grdma_h2.hip", "k_h2_ctl_")
    assert set(seen) == set(KERNELS), sorted(seen)
    for k, v in seen.items():
        assert (v["scratch"], v["vspill"], v["sspill"]) == (0, 0, 0), (k, v)
