"""The mover sweep of tests/test_zz_gpu_movers.py under the wave emulator (tests/cc/wave_emu.h): the same harness source,
tests/cc/mover_sweep.hip, compiled for the CPU, the same reference, the same whole-pool comparison.

This is an EMULATED pass.  The emulator models update_dpp 0x130 / 0x134, the raw buffer loads / stores and their bounds
check; it cannot vouch for the hardware's.  It checks the movers' index arithmetic -- which lane holds which block,
where head, units and tail begin, which tile belongs to which segment -- and the MI355X run of the same lists is what
stands behind the instructions themselves.

Which list: measured on 8 CPUs (a wave is one OS thread and 64 coroutines, sixteen waves per workgroup), the full
one-wave list (168 548 cases) takes 136 s and the 520 plan cases 320 s, the six plans of 16 383 / 16 384 segments
most of it.  Every plan case has to run, so the one-wave part runs the subset built by rule (70 s) -- every alignment
pair at every lane-63 / register / end-of-promise length for copy_g and wave_move_tile, every length at the alignment
pairs (0,0), (0,s), (d,0), (d,d), (d,16-d), every variant without a source pointer in full: 95 202 cases -- and the
file takes six and a half minutes.  Also checked here: the harness kernels compile for gfx950."""
import os
import re
import subprocess

import pytest

from tests import mover_sweep_lib as M

pytestmark = pytest.mark.skipif(not os.path.exists(M.CLANG), reason="needs the ROCm clang++ as host compiler")


@pytest.fixture(scope="module")
def lib():
    return M.build(emulated=True)


@pytest.mark.parametrize("variant", M.VARIANTS)
def test_one_wave_movers_equal_memcpy_under_the_emulator(lib, variant):
    cases = M.tile_cases(variant, subset=True)
    full = M.tile_cases(variant)
    assert set(cases) <= set(full) and len(cases) >= min(len(full), 61 * 30)
    assert M.run_tile_cases(lib, cases, threads=1024) == len(cases)


def test_the_case_lists_have_the_documented_sizes(lib):
    assert sum(len(M.tile_cases(v, subset=True)) for v in M.VARIANTS) == 95202
    assert sum(len(M.tile_cases(v)) for v in M.VARIANTS) == 168548
    assert len(M.plan_cases(lib)) == 520


@pytest.mark.parametrize("tile", [8192, 16384])
@pytest.mark.parametrize("kind", [0, 1, 2])
def test_plans_equal_memcpy_plus_record_tags_under_the_emulator(lib, kind, tile):
    cases = [c for c in M.plan_cases(lib) if c[1] == kind and c[0].tile == tile]
    assert len(cases) == {0: 110, 1: 110, 2: 40}[kind]
    assert sum(M.run_plan_case(lib, p, k, grid) for p, k, grid in cases) == len(cases)


@pytest.mark.skipif(not os.path.exists(M.HIPCC), reason="needs hipcc")
def test_the_harness_kernels_compile_for_gfx950(tmp_path):
    out = tmp_path / "mover_sweep.s"
    p = subprocess.run([M.HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-value", "--cuda-device-only",
                        "-S", M.SRC, "-o", str(out)], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    kernels = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", out.read_text(), re.M))
    assert len(kernels) == 4 and any("k_ms_tiles" in k for k in kernels) and any("k_ms_plan_inline" in k for k in kernels), kernels
    assert sum("k_ms_planILb" in k for k in kernels) == 2, kernels
