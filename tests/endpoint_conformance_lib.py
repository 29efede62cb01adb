"""Runs tests/cc/endpoint_conformance, the reference's endpoint test shape over the vtable mirror, as the device tests
do (tests/test_gpu_endpoint_conformance.py, tests/test_zz_gpu_stats_time.py)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "tests", "cc", "endpoint_conformance")


def run(*args, env=None):
    e = dict(os.environ)
    e.update(env or {})
    p = subprocess.run([HARNESS] + [str(a) for a in args], capture_output=True, text=True, timeout=900, env=e)
    assert p.returncode == 0, p.stdout + p.stderr
    return p.stdout
