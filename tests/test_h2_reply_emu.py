"""CPU suite for the replies framed from descriptors (csrc/grdma_h2_reply.h): its GPU tests under the wave emulator and
its kernels' resources for gfx950."""
import os
import re
import subprocess

import pytest

from tests.test_emu_gpu_suite import CLANG, ROOT, emu_lib, run_gpu_tests  # noqa: F401  (emu_lib is a fixture)

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.mark.skipif(not os.path.exists(CLANG), reason="needs the ROCm clang++ as host compiler")
def test_reply_gpu_tests_under_the_emulator(emu_lib):  # noqa: F811
    # (every test of the file: 22 echo cases and 8 others; about 20 s with 8 workers)
    run_gpu_tests(emu_lib, ["tests/test_zz_gpu_h2_reply.py", "-n", "8"], 30)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_reply_kernels_use_no_scratch(tmp_path):
    src = os.path.join(ROOT, "grpc-rdma_amd", "csrc", "grdma_h2.hip")
    p = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-value", "-c", src,
                        "-o", str(tmp_path / "h2.o"), "-Rpass-analysis=kernel-resource-usage"],
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    cur, seen = None, {}
    for line in p.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = m.group(1) if "k_h2_reply_" in m.group(1) else None
            if cur:
                seen[cur] = {}
            continue
        if cur:
            m = re.search(r"(ScratchSize \[bytes/lane\]|VGPRs Spill|SGPRs Spill): (\d+)", line)
            if m:
                seen[cur][m.group(1)] = int(m.group(2))
    names = {re.search(r"k_h2_reply_[a-z]+", k).group(0) for k in seen}
    assert names == {"k_h2_reply_plan", "k_h2_reply_emit"}
    for k, v in seen.items():
        assert v.get("ScratchSize [bytes/lane]") == 0 and v.get("VGPRs Spill") == 0 and v.get("SGPRs Spill") == 0, (k, v)
