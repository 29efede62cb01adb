"""CPU suite for HTTP/2 on many links (k_h2_frame_links, k_h2_deframe_links, the batch entry and the group pipe): its
GPU tests under the wave emulator and the kernels' resources for gfx950."""
import os
import re
import subprocess

import pytest

from tests.test_emu_gpu_suite import CLANG, ROOT, emu_lib, run_gpu_tests  # noqa: F401  (emu_lib is a fixture)

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.mark.skipif(not os.path.exists(CLANG), reason="needs the ROCm clang++ as host compiler")
def test_links_gpu_tests_under_the_emulator(emu_lib):  # noqa: F811
    # (every test of the file: 3 batch cases, 3 x 2 group-pipe cases, the launch count, the refusals)
    run_gpu_tests(emu_lib, ["tests/test_zz_gpu_h2_links.py", "-n", "4"], 11)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_link_kernels_resources(tmp_path):
    """k_h2_frame_links: no scratch, no spills.  k_h2_deframe_links: no more scratch or spills than k_h2_deframe, the
    kernel it shares its body with, in the SAME compile."""
    src = os.path.join(ROOT, "grpc-rdma_amd", "csrc", "grdma_h2.hip")
    p = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-value", "-c", src,
                        "-o", str(tmp_path / "h2.o"), "-Rpass-analysis=kernel-resource-usage"],
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    cur, seen = None, {}
    for line in p.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            k = re.search(r"k_h2_[a-z_]+?(?=E)", m.group(1))
            cur = k.group(0) if k and k.group(0) in ("k_h2_frame_links", "k_h2_deframe_links", "k_h2_deframe") else None
            if cur:
                seen[cur] = {}
            continue
        if cur:
            m = re.search(r"(ScratchSize \[bytes/lane\]|VGPRs Spill|SGPRs Spill): (\d+)", line)
            if m:
                seen[cur][m.group(1)] = int(m.group(2))
    keys = ("ScratchSize [bytes/lane]", "VGPRs Spill", "SGPRs Spill")
    assert set(seen) == {"k_h2_frame_links", "k_h2_deframe_links", "k_h2_deframe"}, sorted(seen)
    assert all(set(v) == set(keys) for v in seen.values()), seen
    assert [seen["k_h2_frame_links"][k] for k in keys] == [0, 0, 0], seen
    for k in keys:
        assert seen["k_h2_deframe_links"][k] <= seen["k_h2_deframe"][k], (k, seen)
