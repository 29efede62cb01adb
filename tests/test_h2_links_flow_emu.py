"""CPU suite for receive flow control on many links (k_h2_links_fc_*, grdma_h2_fc_account_batch, the group pipe with
ledgers): its GPU tests under the wave emulator and the kernels' resources for gfx950."""
import os

import pytest

from tests.emu_harness import CLANG, emu_lib, run_gpu_tests  # noqa: F401  (emu_lib is a fixture)
from tests.kernel_resources import kernels_of, needs_hipcc

STAGES = ("clear", "keys", "sums", "finish", "emit")


@pytest.mark.skipif(not os.path.exists(CLANG), reason="needs the ROCm clang++ as host compiler")
def test_links_flow_gpu_tests_under_the_emulator(emu_lib):  # noqa: F811
    # (every test of the file: the 5 batch cases, 2 + 2 + 2 x 2 group-pipe cases, the refusals)
    run_gpu_tests(emu_lib, ["tests/test_zz_gpu_h2_links_flow.py", "-n", "4"], 14)


@needs_hipcc
def test_link_ledger_kernels_resources():
    """The five many-link kernels exist, use no scratch and spill nothing, and none takes more VGPRs or LDS than the
    single-transport kernel it shares its source text with, in the same compile."""
    seen = kernels_of("grdma_h2.hip", "k_h2_fc_", "k_h2_links_fc_")
    assert set(seen) == {"k_h2_fc_" + s for s in STAGES} | {"k_h2_links_fc_" + s for s in STAGES}, sorted(seen)
    for k, v in seen.items():
        assert (v["scratch"], v["vspill"], v["sspill"]) == (0, 0, 0), (k, v)
    for s in STAGES:
        one, many = seen["k_h2_fc_" + s], seen["k_h2_links_fc_" + s]
        assert many["vgprs"] <= one["vgprs"] and many["lds"] <= one["lds"], (s, one, many)
