"""CPU suite for the replies on many links (k_h2_reply_plan_links, k_h2_reply_emit_links, grdma_h2_reply_frame_batch,
the group reply pipe): its GPU tests under the wave emulator and the kernels' resources for gfx950."""
import os

import pytest

from tests.emu_harness import CLANG, emu_lib, run_gpu_tests  # noqa: F401  (emu_lib is a fixture)
from tests.kernel_resources import kernels_of, needs_hipcc

NEW = ("k_h2_reply_plan_links", "k_h2_reply_emit_links")
OLD = ("k_h2_reply_plan", "k_h2_reply_emit")


@pytest.mark.skipif(not os.path.exists(CLANG), reason="needs the ROCm clang++ as host compiler")
def test_links_reply_gpu_tests_under_the_emulator(emu_lib):  # noqa: F811
    # (every test of the file: the 3 batch cases, 2 group-reply-pipe cases, the refusals and lifetime)
    run_gpu_tests(emu_lib, ["tests/test_zz_gpu_h2_links_reply.py", "-n", "4"], 6)


@needs_hipcc
def test_link_reply_kernels_resources():
    """The two many-link kernels exist and use no scratch and spill nothing; the two single-transport kernels (the plan
    shares its source text with the many-link plan) still do not either."""
    seen = kernels_of("grdma_h2.hip", "k_h2_reply_")
    assert set(seen) == set(NEW) | set(OLD), sorted(seen)
    for k, v in seen.items():
        assert (v["scratch"], v["vspill"], v["sspill"]) == (0, 0, 0), (k, v)
