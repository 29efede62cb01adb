"""CPU suite for the stream-keyed tables of the HTTP/2 receive path (the parser's stream map, the assembler's carry
table and LDS hash, the ledger's scratch table) under colliding and crowded stream ids: the GPU tests of
tests/test_zz_gpu_h2_stream_tables.py under the wave emulator.  (The emulator runs workgroups one after another: whether
the compare-and-swap claims of the ledger race shows on the device only.)"""
import os

import pytest

from tests.emu_harness import CLANG, emu_lib, run_gpu_tests  # noqa: F401  (emu_lib is a fixture)


@pytest.mark.skipif(not os.path.exists(CLANG), reason="needs the ROCm clang++ as host compiler")
def test_stream_table_gpu_tests_under_the_emulator(emu_lib):  # noqa: F811
    # parser map: 24 orders of a 4-cluster over the wrap (1 case), 50 random orders of eight (5 cases of 10), 10 orders
    # of one cluster on home 0 (1), 100 random client sequences (10 cases of 10), the half-full rule (1), a chunked call
    # on a shifted entry (1); carry table: 24 orders (1), 50 random orders (5 cases of 10); crowded tiles (4), LDS hash
    # collisions and wrap (8), the stream limit (3); ledger: concurrent claims (2), first violator (1), table full (1),
    # unknown ids (1): 45 cases
    run_gpu_tests(emu_lib, ["tests/test_zz_gpu_h2_stream_tables.py", "-n", "4"], 45)
