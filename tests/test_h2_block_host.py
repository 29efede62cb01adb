"""The layout of the HTTP/2 batch block (grpc-rdma_amd/csrc/grdma_h2_block.h) on the CPU: tests/cc/h2_block_host.cc builds
the three layouts of the batch calls, holds every offset against the arithmetic written out again there, and writes every
part into a heap buffer of exactly the reported size -- under the address and undefined-behaviour sanitizers, so an
overrun ends the program."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


@pytest.mark.skipif(not os.path.exists(CLANG), reason="needs the ROCm clang++ as host compiler")
def test_batch_block_layouts_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "h2_block_host")
    subprocess.check_call([CLANG, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "grpc-rdma_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cc", "h2_block_host.cc"), "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert p.stdout.strip().endswith("h2_block_host: ok"), p.stdout[-2000:]
