"""CPU suite for the header decoder on many links (k_h2_links_hpack_*, grdma_h2_hpack_decode_batch): its GPU tests under
the wave emulator and the kernels' resources for gfx950."""
import os

import pytest

from tests.emu_harness import CLANG, emu_lib, run_gpu_tests  # noqa: F401  (emu_lib is a fixture)
from tests.kernel_resources import kernels_of, needs_hipcc

STAGES = ("gather", "copy", "split", "walk", "emit", "commit")


@pytest.mark.skipif(not os.path.exists(CLANG), reason="needs the ROCm clang++ as host compiler")
def test_links_hpack_gpu_tests_under_the_emulator(emu_lib):  # noqa: F811
    # (every test of the file, the 256-link case included: nine links in shuffled order over three calls, batch against
    # single on twin parsers, trouble that stays with its link, 33 and 256 links, uneven links, the refusals, the other
    # followers in both orders: 9 cases)
    run_gpu_tests(emu_lib, ["tests/test_zz_gpu_h2_links_hpack.py", "-n", "4"], 9)


@needs_hipcc
def test_link_hpack_kernels_resources():
    """Exactly the six many-link kernels exist beside the seven single-transport ones, none uses scratch or spills, and
    each takes no more LDS, no lower an occupancy and -- the link lookup aside -- no more VGPRs than the kernel it shares
    its source text with, in the same compile.  The lookup's cost in VGPRs for gfx950 (measured
    against the twins of the same compile: gather 64 = 64, copy 28 = 28, split 42 = 42, walk 99 = 99, emit 24 against 21,
    commit 14 against 12; the occupancy is 8 waves a SIMD on both sides, 2 for the walks): none in the four stages that
    decide the call's time, three registers in the emit and two in the commit, whose link and share of the grid come
    from a division of blockIdx.x."""
    extra = {"emit": 3, "commit": 2}
    seen = kernels_of("grdma_h2.hip", "k_h2_hpack_", "k_h2_links_hpack_")
    assert set(seen) == {"k_h2_hpack_" + s for s in STAGES + ("resize",)} | {"k_h2_links_hpack_" + s for s in STAGES}, sorted(seen)
    for k, v in seen.items():
        assert (v["scratch"], v["vspill"], v["sspill"]) == (0, 0, 0), (k, v)
    for s in STAGES:
        one, many = seen["k_h2_hpack_" + s], seen["k_h2_links_hpack_" + s]
        assert many["vgprs"] <= one["vgprs"] + extra.get(s, 0) and many["lds"] <= one["lds"], (s, one, many)
        assert many["occupancy"] >= one["occupancy"], (s, one, many)
