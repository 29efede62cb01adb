"""CPU suite for the message assembler (csrc/grdma_h2_asm.h): its GPU tests under the wave emulator, its kernels'
resources for gfx950, and the sequential model against the oracle's own message walk."""
import os

import pytest

from tests.emu_harness import CLANG, emu_lib, run_gpu_tests  # noqa: F401  (emu_lib is a fixture)
from tests.kernel_resources import kernels_of, needs_hipcc


@pytest.mark.skipif(not os.path.exists(CLANG), reason="needs the ROCm clang++ as host compiler")
def test_message_assembler_gpu_tests_under_the_emulator(emu_lib):  # noqa: F811
    run_gpu_tests(emu_lib, ["tests/test_zz_gpu_h2_messages.py", "-n", "8", "-k", "not torch_tensor_arena"], 35)


@needs_hipcc
def test_assembler_kernels_use_no_scratch():
    seen = kernels_of("grdma_h2.hip", "k_h2_asm_")
    assert {k for k in seen if not k.endswith("_links")} == {
        "k_h2_asm_tiles", "k_h2_asm_carry", "k_h2_asm_begin", "k_h2_asm_bytes", "k_h2_asm_finish", "k_h2_asm_copy",
        "k_h2_asm_release"}, sorted(seen)
    for k, v in seen.items():
        assert (v["scratch"], v["vspill"], v["sspill"]) == (0, 0, 0), (k, v)


def test_model_against_messages_of_on_the_capture():
    import random
    from oracle import pyorc
    from tests.h2_asm_model import AsmModel, OK, oracle_calls
    from tests.h2_helpers import grpcio_capture, messages_of
    data, exp = grpcio_capture()
    _, ev = pyorc.H2Parser(expect_client_prefix=True).feed(data, cap=len(data) * 4)
    whole = messages_of([e[:5] for e in ev], data)
    assert [b for _, b in whole] == list(exp)
    rng = random.Random(1)
    cuts = sorted(rng.sample(range(1, len(data)), 40))
    bounds = [0] + cuts + [len(data)]
    calls = [[data[a:b]] for a, b in zip(bounds, bounds[1:])]
    m = AsmModel(1 << 20)
    got = []
    for slices, (err, evs) in zip(calls, oracle_calls(calls, prefix=True)):
        got += m.call(evs, slices, err)
        m.release()
    assert all(d[4] == OK for d, _ in got)
    assert [(d[3], b) for d, b in got] == whole
