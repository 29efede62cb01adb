"""CPU suite for the control replies on the device (SETTINGS ACK, PING ACK, RST_STREAM: k_h2_ctl_*, grdma_h2_ctl_*): its
GPU tests under the wave emulator and the kernels' resources for gfx950."""
import os
import re
import subprocess

import pytest

from tests.test_emu_gpu_suite import CLANG, ROOT, emu_lib, run_gpu_tests  # noqa: F401  (emu_lib is a fixture)

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

KERNELS = ("k_h2_ctl_last", "k_h2_ctl_mark", "k_h2_ctl_scan", "k_h2_ctl_emit")


@pytest.mark.skipif(not os.path.exists(CLANG), reason="needs the ROCm clang++ as host compiler")
def test_control_gpu_tests_under_the_emulator(emu_lib):  # noqa: F811
    # (every test of the file: whole frames, 1-byte slices, the capture, PING, SETTINGS and GOAWAY cut between calls,
    # what the peer acknowledged, two GOAWAYs, order, replies spanning both workgroups of the emulator's grid, no control
    # frame, a connection error, lost calls, cap overflows and their repeat, ledger and send windows beside the writer,
    # refusals and lifetime: 30 cases)
    run_gpu_tests(emu_lib, ["tests/test_zz_gpu_h2_control.py", "-n", "4"], 30)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_control_kernels_resources(tmp_path):
    """The four kernels exist and use no scratch and spill nothing."""
    src = os.path.join(ROOT, "grpc-rdma_amd", "csrc", "grdma_h2.hip")
    p = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-value", "-c", src,
                        "-o", str(tmp_path / "h2.o"), "-Rpass-analysis=kernel-resource-usage"],
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    cur, seen = None, {}
    for line in p.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            k = re.search(r"k_h2_ctl_[a-z_]+?(?=E)", m.group(1))
            cur = k.group(0) if k else None
            if cur:
                seen[cur] = {}
            continue
        if cur:
            m = re.search(r"(ScratchSize \[bytes/lane\]|VGPRs Spill|SGPRs Spill): (\d+)", line)
            if m:
                seen[cur][m.group(1)] = int(m.group(2))
    assert set(seen) == set(KERNELS), sorted(seen)
    for k, v in seen.items():
        assert v == {"ScratchSize [bytes/lane]": 0, "VGPRs Spill": 0, "SGPRs Spill": 0}, (k, v)
