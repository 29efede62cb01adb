"""CPU suite for the replies framed from descriptors (csrc/grdma_h2_reply.h): its GPU tests under the wave emulator and
its kernels' resources for gfx950."""
import os

import pytest

from tests.emu_harness import CLANG, emu_lib, run_gpu_tests  # noqa: F401  (emu_lib is a fixture)
from tests.kernel_resources import kernels_of, needs_hipcc


@pytest.mark.skipif(not os.path.exists(CLANG), reason="needs the ROCm clang++ as host compiler")
def test_reply_gpu_tests_under_the_emulator(emu_lib):  # noqa: F811
    # (every test of the file: 22 echo cases and 8 others; about 20 s with 8 workers)
    run_gpu_tests(emu_lib, ["tests/test_zz_gpu_h2_reply.py", "-n", "8"], 30)


@needs_hipcc
def test_reply_kernels_use_no_scratch():
    seen = kernels_of("grdma_h2.hip", "k_h2_reply_")
    assert {k for k in seen if not k.endswith("_links")} == {"k_h2_reply_plan", "k_h2_reply_emit"}, sorted(seen)
    for k, v in seen.items():
        assert (v["scratch"], v["vspill"], v["sspill"]) == (0, 0, 0), (k, v)
