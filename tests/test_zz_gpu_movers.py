"""The byte movers of csrc/grdma_devfn.h on the MI355X, called directly (tests/cc/mover_sweep.hip), against memcpy.

Every payload byte the library moves goes through funnel16, wave_copy_tile, wave_copy_tile_g, wave_zero_tile,
wave_move_tile, tiny_load / tiny_store, plan_tags, plan_tile and run_plan; the pair and HTTP/2 parity tests reach them
only with the alignments and lengths the product's call sites produce.  Here one wave runs one case
{variant, destination alignment, source alignment, length}: all 256 alignment pairs x the lengths at which a mover
changes branch (unit edges, 1..31, lane-63 / register boundaries +-1 / +-16 with and without the head, the end of the
promise and the loop fall-back behind it) -- 168 548 cases -- and 520 plans (one tile per segment, the sampled prefix
search at every stride, record tags in linear and wrapping windows).  The reference is numpy slicing; both pools are
compared whole, byte for byte, so a byte written outside [dst, dst + n) or cleared outside [src, src + n) fails too.
No tolerance.  The case lists and the reference live in tests/mover_sweep_lib.py."""
import pytest

from tests import mover_sweep_lib as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib(gpu):
    return M.build(emulated=False)


@pytest.mark.parametrize("variant", M.VARIANTS)
def test_one_wave_movers_equal_memcpy_at_every_alignment_and_boundary(lib, variant):
    cases = M.tile_cases(variant)
    assert len(cases) >= 16 * 16
    assert M.run_tile_cases(lib, cases) == len(cases)


def test_the_case_lists_have_the_documented_sizes(lib):
    assert sum(len(M.tile_cases(v)) for v in M.VARIANTS) == 168548
    assert len(M.plan_cases(lib)) == 520


@pytest.mark.parametrize("tile", [8192, 16384])
@pytest.mark.parametrize("kind", [0, 1, 2])
def test_plans_equal_memcpy_plus_record_tags(lib, kind, tile):
    cases = [c for c in M.plan_cases(lib) if c[1] == kind and c[0].tile == tile]
    assert len(cases) == {0: 110, 1: 110, 2: 40}[kind]
    assert sum(M.run_plan_case(lib, p, k, grid) for p, k, grid in cases) == len(cases)
