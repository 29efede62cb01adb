"""CPU suite for the metadata reader on many links (k_h2_links_meta_*, grdma_h2_meta_read_batch): its GPU tests under the
wave emulator and the kernels' resources for gfx950."""
import os

import pytest

from tests.emu_harness import CLANG, emu_lib, run_gpu_tests  # noqa: F401  (emu_lib is a fixture)
from tests.kernel_resources import kernels_of, needs_hipcc

STAGES = ("fields", "blocks", "emit")


@pytest.mark.skipif(not os.path.exists(CLANG), reason="needs the ROCm clang++ as host compiler")
def test_links_meta_gpu_tests_under_the_emulator(emu_lib):  # noqa: F811
    # (every test of the file, the 1025-block and the 256-item case included: 0 to 1025 blocks and 1023 to 1025 fields in
    # a link between two small ones, a first known key in the second step, compaction inside its link, batch against
    # single on twin readers, nine links in shuffled order over three calls, trouble that stays with its item, one input
    # for sixteen items, 33 and 256 items, an empty item, decode -> read -> encode on three links, refusals and lifetime:
    # 27 cases.  Under the emulator a link has two workgroups, not four.)
    run_gpu_tests(emu_lib, ["tests/test_zz_gpu_h2_links_meta.py", "-n", "4"], 27)


@needs_hipcc
def test_link_meta_kernels_resources():
    """Exactly the three many-link kernels exist beside the three single-call ones the header names, and each has no
    scratch, no spills and far less than 64 KiB of LDS."""
    seen = kernels_of("grdma_h2.hip", "k_h2_meta_", "k_h2_links_meta_")
    assert set(seen) == {"k_h2_meta_" + s for s in STAGES} | {"k_h2_links_meta_" + s for s in STAGES}, sorted(seen)
    for k, v in seen.items():
        assert (v["scratch"], v["vspill"], v["sspill"]) == (0, 0, 0), (k, v)
        assert v["lds"] < 65536, (k, v)
