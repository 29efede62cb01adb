"""CPU suite for the call-metadata reader on the device (k_h2_meta_*, grdma_h2_meta_*): its GPU tests under the wave
emulator and the kernels' resources for gfx950."""
import os

import pytest

from tests.emu_harness import CLANG, emu_lib, run_gpu_tests  # noqa: F401  (emu_lib is a fixture)
from tests.kernel_resources import kernels_of, needs_hipcc

KERNELS = ("k_h2_meta_fields", "k_h2_meta_blocks", "k_h2_meta_emit")


@pytest.mark.skipif(not os.path.exists(CLANG), reason="needs the ROCm clang++ as host compiler")
def test_meta_gpu_tests_under_the_emulator(emu_lib):  # noqa: F811
    # (every test of the file: the block counts around a workgroup's run and beyond the grid, 0 to 257 fields per block,
    # a pseudo-header behind a regular field and a second :path at the edges of a step, the first grpc-timeout across
    # steps, every known key and its neighbours, every byte value in a value and in a name, the method table empty, full,
    # colliding and at the longest path, every verdict, the statuses, shared fields, the rejection list, the two caps and
    # their repeat, the three kinds of bad input, refusals and lifetime, decode -> read -> encode: 50 cases)
    run_gpu_tests(emu_lib, ["tests/test_zz_gpu_h2_meta.py", "-n", "4"], 50)


@needs_hipcc
def test_meta_kernels_resources():
    """Exactly the three kernels exist, each with no scratch and no spills and far less than 64 KiB of LDS."""
    seen = kernels_of("grdma_h2.hip", "k_h2_meta_")
    assert set(seen) == set(KERNELS), sorted(seen)
    for k, v in seen.items():
        assert (v["scratch"], v["vspill"], v["sspill"]) == (0, 0, 0), (k, v)
        assert v["lds"] < 65536, (k, v)
