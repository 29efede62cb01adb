"""CPU suite for the call table on the device (k_h2_calls_*, grdma_h2_calls_*): its GPU tests under the wave emulator
and the kernels' resources for gfx950."""
import os

import pytest

from tests.emu_harness import CLANG, emu_lib, run_gpu_tests  # noqa: F401  (emu_lib is a fixture)
from tests.kernel_resources import kernels_of, needs_hipcc

KERNELS = ("k_h2_calls_clear", "k_h2_calls_claim", "k_h2_calls_wins", "k_h2_calls_insert", "k_h2_calls_msgs", "k_h2_calls_cols",
           "k_h2_calls_finish", "k_h2_calls_emit")


@pytest.mark.skipif(not os.path.exists(CLANG), reason="needs the ROCm clang++ as host compiler")
def test_calls_gpu_tests_under_the_emulator(emu_lib):  # noqa: F811
    # (every test of the file: record, message and event counts around a wave, a workgroup's 256 and a run and beyond
    # the grid; no method, one, 4096; everything orphaned; sixteen slots clustered on the wrap, opens and LEFTs in every
    # order of a cluster, half the slots and one more; a stream across tiles and steps, LAST; duplicates at the lanes'
    # edges and across steps; the orphan checks' order, expiry order, both caps and their repeat, bad input, refusals and
    # lifetime, deframe -> decode -> read -> route on device tables: 73 cases)
    run_gpu_tests(emu_lib, ["tests/test_zz_gpu_h2_calls.py", "-n", "4"], 73)


@needs_hipcc
def test_calls_kernels_resources():
    """Exactly the eight kernels exist, each with no scratch and no spills and far less than 64 KiB of LDS."""
    seen = kernels_of("grdma_h2.hip", "k_h2_calls_")
    assert set(seen) == set(KERNELS), sorted(seen)
    for k, v in seen.items():
        assert (v["scratch"], v["vspill"], v["sspill"]) == (0, 0, 0), (k, v)
        assert v["lds"] < 65536, (k, v)
