"""CPU suite for the header encoder on many links (k_h2_links_hpenc_*, grdma_h2_hpenc_encode_batch): its GPU tests under
the wave emulator and the kernels' resources for gfx950."""
import os

import pytest

from tests.emu_harness import CLANG, emu_lib, run_gpu_tests  # noqa: F401  (emu_lib is a fixture)
from tests.kernel_resources import kernels_of, needs_hipcc

STAGES = ("scan", "walk", "emit", "commit")


@pytest.mark.skipif(not os.path.exists(CLANG), reason="needs the ROCm clang++ as host compiler")
def test_links_hpenc_gpu_tests_under_the_emulator(emu_lib):  # noqa: F811
    # (every test of the file, the 256-link case included: nine links in shuffled order over three calls, batch against
    # single on twin encoders, trouble that stays with its link and the second run, per-link peer settings, uneven
    # links, 33 and 256 links, one input for many links, the decoders' output forwarded, the refusals: 10 cases)
    run_gpu_tests(emu_lib, ["tests/test_zz_gpu_h2_links_hpenc.py", "-n", "4"], 10)


@needs_hipcc
def test_link_hpenc_kernels_resources():
    """Exactly the four many-link kernels exist beside the four single-connection ones, none uses scratch or spills, and
    each takes no more LDS, no lower an occupancy and -- the link lookup aside -- no more VGPRs than the kernel it shares
    its source text with, in the same compile.  The lookup's cost in VGPRs for gfx950 (measured against the twins of the
    same compile: scan 50 against 51, walk 71 against 70, emit 34 = 34, commit 15 against 10; the occupancy is 8 waves a
    SIMD on both sides, 3 for the walks, whose 51296 bytes of LDS bound it): none in the scan and the emit, one register
    in the walk, which carries the call and holds three pointers from the table where its twin derives them from one,
    and five in the commit, a loop of a dozen instructions whose link and share of the grid come from a division of
    blockIdx.x and whose twin folds its stride into a constant."""
    extra = {"walk": 1, "commit": 5}
    seen = kernels_of("grdma_h2.hip", "k_h2_hpenc_", "k_h2_links_hpenc_")
    assert set(seen) == {"k_h2_hpenc_" + s for s in STAGES} | {"k_h2_links_hpenc_" + s for s in STAGES}, sorted(seen)
    for k, v in seen.items():
        assert (v["scratch"], v["vspill"], v["sspill"]) == (0, 0, 0), (k, v)
    for s in STAGES:
        one, many = seen["k_h2_hpenc_" + s], seen["k_h2_links_hpenc_" + s]
        assert many["vgprs"] <= one["vgprs"] + extra.get(s, 0) and many["lds"] <= one["lds"], (s, one, many)
        assert many["occupancy"] >= one["occupancy"], (s, one, many)
