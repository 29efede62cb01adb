"""CPU suite for the replies under the peer's windows (k_h2_wr_*, grdma_h2_reply_frame_windowed): its GPU tests under
the wave emulator and the kernels' resources for gfx950."""
import os

import pytest

from tests.emu_harness import CLANG, emu_lib, run_gpu_tests  # noqa: F401  (emu_lib is a fixture)
from tests.kernel_resources import kernels_of, needs_hipcc

STAGES = ("queue", "commit")


@pytest.mark.skipif(not os.path.exists(CLANG), reason="needs the ROCm clang++ as host compiler")
def test_windowed_reply_gpu_tests_under_the_emulator(emu_lib):  # noqa: F811
    # (every test of the file: open windows against a twin at three frame sizes, a stream window and the rest, four
    # small windows, the connection window and old entries in front, the inlined run, statuses and routes, a reset,
    # SETTINGS between two pieces, the ring's wrap, the overflows, 4096 messages, a skipped call, a send-windows call
    # in between, the echo round trip, refusals and lifetime: 20 cases)
    run_gpu_tests(emu_lib, ["tests/test_zz_gpu_h2_windowed_reply.py", "-n", "4"], 20)


@needs_hipcc
def test_windowed_reply_kernels_resources():
    """Exactly the four new kernels exist under the new prefixes, and none uses scratch or spills."""
    seen = kernels_of("grdma_h2.hip", "k_h2_wr_", "k_h2_links_wr_")
    assert set(seen) == {"k_h2_wr_" + s for s in STAGES} | {"k_h2_links_wr_" + s for s in STAGES}, sorted(seen)
    for k, v in seen.items():
        assert (v["scratch"], v["vspill"], v["sspill"]) == (0, 0, 0), (k, v)
