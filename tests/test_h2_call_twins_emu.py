"""CPU suite for the shared per-item steps of the HTTP/2 host calls (csrc/grdma_h2_host_calls.inc): the twins test under
the wave emulator."""
import os

import pytest

from tests.emu_harness import CLANG, emu_lib, run_gpu_tests  # noqa: F401  (emu_lib is a fixture)


@pytest.mark.skipif(not os.path.exists(CLANG), reason="needs the ROCm clang++ as host compiler")
def test_call_twins_gpu_tests_under_the_emulator(emu_lib):  # noqa: F811
    # (the refusals and the batch of one against the single call, for the ledger's account, the send windows' intake and
    # framing, the control replies and the windowed reply: 10 cases)
    run_gpu_tests(emu_lib, ["tests/test_zz_gpu_h2_call_twins.py", "-n", "4"], 10)
