"""The emulator harness of the CPU suite: the product sources compiled over the wave emulator and the HIP API stand-in
(tests/cc/wave_emu.h, tests/cc/hip_api_emu.h, tests/cc/build_emu.sh -> oracle/_build/libgrdma_emu.so), loaded in place of
libgrdma_amd.so (GRDMA_LIB_PATH), and `-m gpu` tests run against it in a child pytest.  tests/test_emu_gpu_suite.py and
the tests/test_*_emu.py files are its users.  `emu_lib` is a fixture: a module that uses it imports it by name
(`# noqa: F401`) and its tests take it as an argument (`# noqa: F811`).

The rules of this directory's helper modules:
* No module imports a `test_*` module.  What two files need lives in a library: this one, tests/kernel_resources.py,
  tests/pair_lib.py, tests/stream_job_lib.py, tests/endpoint_conformance_lib.py, the tests/h2_*_lib.py and
  tests/*_sweep_lib.py files.
* Siblings are imported through the package: `from tests.<module> import ...` or `from tests import <module> as X`, also
  in the `*_subset.py` files a child pytest collects.  (conftest.py puts this directory itself on sys.path as well; a
  bare `import <module>` would load the same file a second time, with its caches and constants.)
* What the compiler allocated to a kernel comes from tests/kernel_resources.py::report: one compile per unit and
  process, one parser."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
EMU_SO = os.path.join(ROOT, "oracle", "_build", "libgrdma_emu.so")


@pytest.fixture(scope="module")
def emu_lib(built):
    srcs = []
    for d in (os.path.join(ROOT, "grpc-rdma_amd", "csrc"), os.path.join(ROOT, "tests", "cc"), os.path.join(ROOT, "include")):
        srcs += [os.path.join(d, f) for f in os.listdir(d) if f.endswith((".hip", ".cc", ".h", ".hpp", ".sh", ".inc"))]
    if not os.path.exists(EMU_SO) or any(os.path.getmtime(s) > os.path.getmtime(EMU_SO) for s in srcs):
        subprocess.check_call(["bash", os.path.join(ROOT, "tests", "cc", "build_emu.sh")], stdout=subprocess.DEVNULL,
                              stderr=subprocess.DEVNULL)
    return EMU_SO


def run_gpu_tests(emu_lib, args, min_passed):
    env = dict(os.environ, GRDMA_LIB_PATH=emu_lib, GRDMA_TEST_NEW="1", GRDMA_TEST_ALLOW_EMU="1")
    cmd = [sys.executable, "-m", "pytest", "-m", "gpu", "-q", "-x", "-p", "no:cacheprovider", "--timeout", "600"] + args
    last = ""
    for attempt in range(2):  # (the staging waves of the deframer are real threads: one retry on a scheduling hiccup)
        p = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=1500)
        last = (p.stdout + p.stderr)[-3000:]
        if p.returncode == 0:
            tail = p.stdout.strip().splitlines()[-1]
            n = int(tail.split(" passed")[0].split()[-1])
            assert n >= min_passed, tail
            return
    raise AssertionError(last)
