"""CPU suite for the call table on many links (k_h2_links_calls_*, grdma_h2_calls_step_batch): its GPU tests under the wave
emulator and the kernels' resources for gfx950."""
import os

import pytest

from tests.emu_harness import CLANG, emu_lib, run_gpu_tests  # noqa: F401  (emu_lib is a fixture)
from tests.kernel_resources import kernels_of, needs_hipcc

STAGES = ("clear", "claim", "wins", "insert", "msgs", "cols", "finish", "emit")


@pytest.mark.skipif(not os.path.exists(CLANG), reason="needs the ROCm clang++ as host compiler")
def test_links_calls_gpu_tests_under_the_emulator(emu_lib):  # noqa: F811
    # (every test of the file, the 2049-count and the 256-item case included: record, message and event counts of 0 to
    # 2049 in a link between two small ones, a stream in every run of its link over two batches, duplicates across a
    # run's edge and across steps, 0, 1 and 4096 methods, everything orphaned, half of sixteen slots and one more, a
    # cluster on the wrap, twin tables stepped singly and in batches with the roles swapped, nine links in shuffled
    # order over three batches, trouble that stays with its item and its repeat, a batch in which nothing commits, an
    # empty item against its deadline, per-item clocks, one input for sixteen items, 33 and 256 items, deframe -> decode
    # batch -> read batch -> route on three links, refusals and lifetime: 33 cases.  Under the emulator a link has two
    # workgroups, not four.)
    run_gpu_tests(emu_lib, ["tests/test_zz_gpu_h2_links_calls.py", "-n", "4"], 33)


@needs_hipcc
def test_link_calls_kernels_resources():
    """Exactly the eight many-link kernels carry the prefix, and each has no scratch, no spills and less than 64 KiB of
    LDS."""
    seen = kernels_of("grdma_h2.hip", "k_h2_links_calls_")
    assert set(seen) == {"k_h2_links_calls_" + s for s in STAGES}, sorted(seen)
    for k, v in seen.items():
        assert (v["scratch"], v["vspill"], v["sspill"]) == (0, 0, 0), (k, v)
        assert v["lds"] < 65536, (k, v)
