"""CPU suite for the message assembler on many links (k_h2_asm_*_links, grdma_h2_deframe_messages_batch, the group pipe
with assemblers): its GPU tests under the wave emulator and the kernels' resources for gfx950."""
import os

import pytest

from tests.emu_harness import CLANG, emu_lib, run_gpu_tests  # noqa: F401  (emu_lib is a fixture)
from tests.kernel_resources import kernels_of, needs_hipcc

NEW = ("k_h2_asm_tiles_links", "k_h2_asm_carry_links", "k_h2_asm_begin_links", "k_h2_asm_bytes_links",
       "k_h2_asm_finish_links", "k_h2_asm_copy_links", "k_h2_asm_release_links")
OLD = ("k_h2_asm_tiles", "k_h2_asm_carry", "k_h2_asm_begin", "k_h2_asm_bytes", "k_h2_asm_finish", "k_h2_asm_copy",
       "k_h2_asm_release")


@pytest.mark.skipif(not os.path.exists(CLANG), reason="needs the ROCm clang++ as host compiler")
def test_links_messages_gpu_tests_under_the_emulator(emu_lib):  # noqa: F811
    # (every test of the file: the 4 batch cases, 2 x 2 + 2 group-pipe cases, the refusals)
    run_gpu_tests(emu_lib, ["tests/test_zz_gpu_h2_links_messages.py", "-n", "4"], 11)


@needs_hipcc
def test_link_assembler_kernels_resources():
    """The seven many-link kernels exist and use no scratch and spill nothing; the seven single-transport kernels they
    share their source text with still do not either."""
    seen = kernels_of("grdma_h2.hip", "k_h2_asm_")
    assert set(seen) == set(NEW) | set(OLD), sorted(seen)
    for k, v in seen.items():
        assert (v["scratch"], v["vspill"], v["sspill"]) == (0, 0, 0), (k, v)
