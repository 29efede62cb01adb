"""CPU suite for receive flow control on the device (the window ledger: k_h2_fc_*, grdma_h2_fc_*,
grdma_h2_pipe_attach_flow_control): its GPU tests under the wave emulator and the kernels' resources for gfx950."""
import os

import pytest

from tests.emu_harness import CLANG, emu_lib, run_gpu_tests  # noqa: F401  (emu_lib is a fixture)
from tests.kernel_resources import kernels_of, needs_hipcc

KERNELS = ("k_h2_fc_clear", "k_h2_fc_keys", "k_h2_fc_sums", "k_h2_fc_finish", "k_h2_fc_emit")


@pytest.mark.skipif(not os.path.exists(CLANG), reason="needs the ROCm clang++ as host compiler")
def test_flow_control_gpu_tests_under_the_emulator(emu_lib):  # noqa: F811
    # (every test of the file: standalone client and server side, violations, round trip, assembler, pipe fused and
    # unfused, the chunked deframer, refusals and lifetime: 17 cases)
    run_gpu_tests(emu_lib, ["tests/test_zz_gpu_h2_flow.py", "-n", "4"], 17)


@needs_hipcc
def test_flow_control_kernels_resources():
    """The ledger's five kernels exist and use no scratch and spill nothing."""
    seen = kernels_of("grdma_h2.hip", "k_h2_fc_")
    assert set(seen) == set(KERNELS), sorted(seen)
    for k, v in seen.items():
        assert (v["scratch"], v["vspill"], v["sspill"]) == (0, 0, 0), (k, v)
