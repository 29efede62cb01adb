"""The layout of the batch block of grdma_h2_calls_step_batch (grpc-rdma_amd/csrc/grdma_h2_block.h: h2_calls_block_layout)
on the CPU: tests/cc/h2_calls_block_host.cc builds it for 1 to GRDMA_H2_BATCH_MAX items, holds every offset against the
arithmetic written out again there, and writes every part into heap buffers of exactly the reported sizes -- under the
address and undefined-behaviour sanitizers, so an overrun ends the program."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


@pytest.mark.skipif(not os.path.exists(CLANG), reason="needs the ROCm clang++ as host compiler")
def test_calls_batch_block_layout_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "h2_calls_block_host")
    subprocess.check_call([CLANG, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "grpc-rdma_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cc", "h2_calls_block_host.cc"), "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert p.stdout.strip().endswith("h2_calls_block_host: ok"), p.stdout[-2000:]
