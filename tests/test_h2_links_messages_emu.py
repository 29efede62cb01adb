"""CPU suite for the message assembler on many links (k_h2_asm_*_links, grdma_h2_deframe_messages_batch, the group pipe
with assemblers): its GPU tests under the wave emulator and the kernels' resources for gfx950."""
import os
import re
import subprocess

import pytest

from tests.test_emu_gpu_suite import CLANG, ROOT, emu_lib, run_gpu_tests  # noqa: F401  (emu_lib is a fixture)

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

NEW = ("k_h2_asm_tiles_links", "k_h2_asm_carry_links", "k_h2_asm_begin_links", "k_h2_asm_bytes_links",
       "k_h2_asm_finish_links", "k_h2_asm_copy_links", "k_h2_asm_release_links")
OLD = ("k_h2_asm_tiles", "k_h2_asm_carry", "k_h2_asm_begin", "k_h2_asm_bytes", "k_h2_asm_finish", "k_h2_asm_copy",
       "k_h2_asm_release")


@pytest.mark.skipif(not os.path.exists(CLANG), reason="needs the ROCm clang++ as host compiler")
def test_links_messages_gpu_tests_under_the_emulator(emu_lib):  # noqa: F811
    # (every test of the file: the 4 batch cases, 2 x 2 + 2 group-pipe cases, the refusals)
    run_gpu_tests(emu_lib, ["tests/test_zz_gpu_h2_links_messages.py", "-n", "4"], 11)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_link_assembler_kernels_resources(tmp_path):
    """The seven many-link kernels exist and use no scratch and spill nothing; the seven single-transport kernels they
    share their source text with still do not either."""
    src = os.path.join(ROOT, "grpc-rdma_amd", "csrc", "grdma_h2.hip")
    p = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-value", "-c", src,
                        "-o", str(tmp_path / "h2.o"), "-Rpass-analysis=kernel-resource-usage"],
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    cur, seen = None, {}
    for line in p.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            k = re.search(r"k_h2_asm_[a-z_]+?(?=E)", m.group(1))
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
