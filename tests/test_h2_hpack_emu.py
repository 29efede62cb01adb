"""CPU suite for the header decoder on the device (HPACK: k_h2_hpack_*, grdma_h2_hpack_*): its GPU tests under the wave
emulator and the kernels' resources for gfx950."""
import os

import pytest

from tests.emu_harness import CLANG, emu_lib, run_gpu_tests  # noqa: F401  (emu_lib is a fixture)
from tests.kernel_resources import kernels_of, needs_hipcc

KERNELS = ("k_h2_hpack_gather", "k_h2_hpack_copy", "k_h2_hpack_split", "k_h2_hpack_walk", "k_h2_hpack_emit", "k_h2_hpack_commit",
           "k_h2_hpack_resize")


@pytest.mark.skipif(not os.path.exists(CLANG), reason="needs the ROCm clang++ as host compiler")
def test_hpack_gpu_tests_under_the_emulator(emu_lib):  # noqa: F811
    # (every test of the file: the capture whole, in 1-byte slices and cut between calls, a block cut at every byte,
    # padding and priority, the padding errors, CONTINUATIONs, DATA between blocks and a refused stream, 300 blocks,
    # references across blocks and calls, prefix edges, Huffman and its errors, the table filled to the byte, oversized
    # entries, size updates, RFC 7541 4.4, the setting lowered, malformed blocks, max_block_bytes, an error in the third
    # block of five, the three cap overflows and their repeat, lost and skipped calls, the control writer and the send
    # windows beside the decoder, refusals and lifetime: 45 cases)
    run_gpu_tests(emu_lib, ["tests/test_zz_gpu_h2_hpack.py", "-n", "4"], 45)


@needs_hipcc
def test_hpack_kernels_resources():
    """Exactly the seven kernels exist, each with no scratch and no spills."""
    seen = kernels_of("grdma_h2.hip", "k_h2_hpack_")
    assert set(seen) == set(KERNELS), sorted(seen)
    for k, v in seen.items():
        assert (v["scratch"], v["vspill"], v["sspill"]) == (0, 0, 0), (k, v)
