"""CPU suite for the message assembler (csrc/grdma_h2_asm.h): its GPU tests under the wave emulator, its kernels'
resources for gfx950, and the sequential model against the oracle's own message walk."""
import os
import re
import subprocess

import pytest

from tests.test_emu_gpu_suite import CLANG, ROOT, emu_lib, run_gpu_tests  # noqa: F401  (emu_lib is a fixture)

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.mark.skipif(not os.path.exists(CLANG), reason="needs the ROCm clang++ as host compiler")
def test_message_assembler_gpu_tests_under_the_emulator(emu_lib):  # noqa: F811
    run_gpu_tests(emu_lib, ["tests/test_zz_gpu_h2_messages.py", "-n", "8", "-k", "not torch_tensor_arena"], 35)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_assembler_kernels_use_no_scratch(tmp_path):
    src = os.path.join(ROOT, "grpc-rdma_amd", "csrc", "grdma_h2.hip")
    p = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-value", "-c", src,
                        "-o", str(tmp_path / "h2.o"), "-Rpass-analysis=kernel-resource-usage"],
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    cur, seen = None, {}
    for line in p.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = m.group(1) if "k_h2_asm_" in m.group(1) else None
            if cur:
                seen[cur] = {}
            continue
        if cur:
            m = re.search(r"(ScratchSize \[bytes/lane\]|VGPRs Spill|SGPRs Spill): (\d+)", line)
            if m:
                seen[cur][m.group(1)] = int(m.group(2))
    names = {re.search(r"k_h2_asm_[a-z]+", k).group(0) for k in seen}
    assert names == {"k_h2_asm_tiles", "k_h2_asm_carry", "k_h2_asm_begin", "k_h2_asm_bytes", "k_h2_asm_finish",
                     "k_h2_asm_copy", "k_h2_asm_release"}
    for k, v in seen.items():
        assert v.get("ScratchSize [bytes/lane]") == 0 and v.get("VGPRs Spill") == 0 and v.get("SGPRs Spill") == 0, (k, v)


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
