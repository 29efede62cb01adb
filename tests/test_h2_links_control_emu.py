"""CPU suite for the control replies on many links (k_h2_links_ctl_*, grdma_h2_ctl_reply_batch): its GPU tests under the
wave emulator and the kernels' resources for gfx950."""
import os
import re
import subprocess

import pytest

from tests.test_emu_gpu_suite import CLANG, ROOT, emu_lib, run_gpu_tests  # noqa: F401  (emu_lib is a fixture)

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

STAGES = ("last", "mark", "scan", "emit")
FIELDS = {"ScratchSize [bytes/lane]": "scratch", "VGPRs Spill": "vspill", "SGPRs Spill": "sspill", "VGPRs": "vgprs",
          "LDS Size [bytes/block]": "lds"}


@pytest.mark.skipif(not os.path.exists(CLANG), reason="needs the ROCm clang++ as host compiler")
def test_links_control_gpu_tests_under_the_emulator(emu_lib):  # noqa: F811
    # (every test of the file, the 256-link case included: nine links in shuffled order over two calls, batch against
    # single on twin parsers, trouble that stays with its link, 256 links and the refusals: 4 cases)
    run_gpu_tests(emu_lib, ["tests/test_zz_gpu_h2_links_control.py", "-n", "4"], 4)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_link_control_kernels_resources(tmp_path):
    """The four many-link kernels exist beside their single-transport twins, none uses scratch or spills, and each takes
    no more VGPRs or LDS than the kernel it shares its source text with, in the same compile."""
    src = os.path.join(ROOT, "grpc-rdma_amd", "csrc", "grdma_h2.hip")
    p = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-value", "-c", src,
                        "-o", str(tmp_path / "h2.o"), "-Rpass-analysis=kernel-resource-usage"],
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    cur, seen = None, {}
    for line in p.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            k = re.search(r"k_h2_(?:links_)?ctl_[a-z]+?(?=E)", m.group(1))
            cur = k.group(0) if k else None
            if cur:
                seen[cur] = {}
            continue
        if cur:
            m = re.search(r"remark:\s+(ScratchSize \[bytes/lane\]|VGPRs Spill|SGPRs Spill|VGPRs|LDS Size \[bytes/block\]): (\d+)", line)
            if m:
                seen[cur][FIELDS[m.group(1)]] = int(m.group(2))
    assert set(seen) == {"k_h2_ctl_" + s for s in STAGES} | {"k_h2_links_ctl_" + s for s in STAGES}, sorted(seen)
    for k, v in seen.items():
        assert set(v) == set(FIELDS.values()), (k, v)
        assert (v["scratch"], v["vspill"], v["sspill"]) == (0, 0, 0), (k, v)
    for s in STAGES:
        one, many = seen["k_h2_ctl_" + s], seen["k_h2_links_ctl_" + s]
        assert many["vgprs"] <= one["vgprs"] and many["lds"] <= one["lds"], (s, one, many)
