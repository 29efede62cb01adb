"""CPU suite for the replies on many links (k_h2_reply_plan_links, k_h2_reply_emit_links, grdma_h2_reply_frame_batch,
the group reply pipe): its GPU tests under the wave emulator and the kernels' resources for gfx950."""
import os
import re
import subprocess

import pytest

from tests.test_emu_gpu_suite import CLANG, ROOT, emu_lib, run_gpu_tests  # noqa: F401  (emu_lib is a fixture)

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

NEW = ("k_h2_reply_plan_links", "k_h2_reply_emit_links")
OLD = ("k_h2_reply_plan", "k_h2_reply_emit")


@pytest.mark.skipif(not os.path.exists(CLANG), reason="needs the ROCm clang++ as host compiler")
def test_links_reply_gpu_tests_under_the_emulator(emu_lib):  # noqa: F811
    # (every test of the file: the 3 batch cases, 2 group-reply-pipe cases, the refusals and lifetime)
    run_gpu_tests(emu_lib, ["tests/test_zz_gpu_h2_links_reply.py", "-n", "4"], 6)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_link_reply_kernels_resources(tmp_path):
    """The two many-link kernels exist and use no scratch and spill nothing; the two single-transport kernels (the plan
    shares its source text with the many-link plan) still do not either."""
    src = os.path.join(ROOT, "grpc-rdma_amd", "csrc", "grdma_h2.hip")
    p = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-value", "-c", src,
                        "-o", str(tmp_path / "h2.o"), "-Rpass-analysis=kernel-resource-usage"],
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    cur, seen = None, {}
    for line in p.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            k = re.search(r"k_h2_reply_[a-z_]+?(?=E)", m.group(1))
            cur = k.group(0) if k else None
            if cur:
                seen[cur] = {}
            continue
        if cur:
            m = re.search(r"(ScratchSize \[bytes/lane\]|VGPRs Spill|SGPRs Spill): (\d+)", line)
            if m:
                seen[cur][m.group(1)] = int(m.group(2))
    assert set(seen) == set(NEW) | set(OLD), sorted(seen)
    for k, v in seen.items():
        assert v == {"ScratchSize [bytes/lane]": 0, "VGPRs Spill": 0, "SGPRs Spill": 0}, (k, v)
