"""CPU suite for send flow control on the device (the peer's windows and the framer under them: k_h2_sw_*,
grdma_h2_sw_*): its GPU tests under the wave emulator and the kernels' resources for gfx950."""
import os

import pytest

from tests.emu_harness import CLANG, emu_lib, run_gpu_tests  # noqa: F401  (emu_lib is a fixture)
from tests.kernel_resources import kernels_of, needs_hipcc

KERNELS = ("k_h2_sw_clear", "k_h2_sw_take", "k_h2_sw_finish", "k_h2_sw_plan", "k_h2_sw_emit")


@pytest.mark.skipif(not os.path.exists(CLANG), reason="needs the ROCm clang++ as host compiler")
def test_send_window_gpu_tests_under_the_emulator(emu_lib):  # noqa: F811
    # (every test of the file: intake whole, spread and cut, settings, violations, lost calls, colliding streams, the
    # table, the capture; the framer at open windows, at the windows' edges, resumed, at 4096 messages and 2048 streams,
    # cap overflows, refusals; the round trip with the ledger: 70 cases)
    run_gpu_tests(emu_lib, ["tests/test_zz_gpu_h2_send_window.py", "-n", "4"], 70)


@needs_hipcc
def test_send_window_kernels_resources():
    """The five kernels exist and use no scratch and spill nothing."""
    seen = kernels_of("grdma_h2.hip", "k_h2_sw_")
    assert set(seen) == set(KERNELS), sorted(seen)
    for k, v in seen.items():
        assert (v["scratch"], v["vspill"], v["sspill"]) == (0, 0, 0), (k, v)
