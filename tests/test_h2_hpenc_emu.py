"""CPU suite for the header encoder on the device (HPACK, sending: k_h2_hpenc_*, grdma_h2_hpenc_*): its GPU tests under the
wave emulator and the kernels' resources for gfx950."""
import os

import pytest

from tests.emu_harness import CLANG, emu_lib, run_gpu_tests  # noqa: F401  (emu_lib is a fixture)
from tests.kernel_resources import kernels_of, needs_hipcc

KERNELS = ("k_h2_hpenc_scan", "k_h2_hpenc_walk", "k_h2_hpenc_emit", "k_h2_hpenc_commit")


@pytest.mark.skipif(not os.path.exists(CLANG), reason="needs the ROCm clang++ as host compiler")
def test_hpenc_gpu_tests_under_the_emulator(emu_lib):  # noqa: F811
    # (every test of the file: RFC 7541 C.4 and C.6, one field per block, the prefix edges of indices, name indices and
    # string lengths, every byte value, Huffman against raw, the padding's alignments, references inside a block, across
    # blocks and calls, an insertion that evicts a later field's match, entries of the table's size and one more, size 0,
    # the ring at its most entries, the byte ring across its wrap, colliding hashes, the walk's steps, 300 blocks, an
    # empty block, zero blocks, a run of 300 empty blocks, blocks around the frame size, fields cut by a frame, set_peer,
    # size updates, the two caps and their repeat, the five kinds of bad input, the decoder's output forwarded, refusals
    # and lifetime: 41 cases)
    run_gpu_tests(emu_lib, ["tests/test_zz_gpu_h2_hpenc.py", "-n", "4"], 41)


@needs_hipcc
def test_hpenc_kernels_resources():
    """Exactly the four kernels exist, each with no scratch and no spills; the walk's table stays under 64 KiB of LDS."""
    seen = kernels_of("grdma_h2.hip", "k_h2_hpenc_")
    assert set(seen) == set(KERNELS), sorted(seen)
    for k, v in seen.items():
        assert (v["scratch"], v["vspill"], v["sspill"]) == (0, 0, 0), (k, v)
    assert seen["k_h2_hpenc_walk"]["lds"] < 65536, seen["k_h2_hpenc_walk"]
