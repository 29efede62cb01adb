"""The stream-job planners (rxf_body / txf_body on the sequential schedule; rxm_body / rxh_body / txm_body on the paired one,
the general planners behind them) swept over record patterns built from the constants they branch on, against the oracle:
delivered slices, round count, ring image and state exact, and per family whether the steady-state bodies take the drains
or decline them by the named reason.  One function per family, every case of it in a loop; the failing case is in the
assertion message.  Cases, witnesses and driver: tests/planner_sweep_lib.py.

Every case's witnesses are checked from the oracle alone when this module is imported: a case that does not reach the
edge it is there for fails the collection, on any machine, before anything runs on a device."""
import pytest

from tests import planner_sweep_lib as L

pytestmark = pytest.mark.gpu

for _fam in sorted(L.FAMILIES):
    for _case in L.cases(_fam):
        L.check_witnesses(_case)

grid = pytest.mark.parametrize("schedule,wire", [(s, w) for s in L.SCHEDULES for w in L.WIRES],
                               ids=["%s-%s" % (s, w) for s in L.SCHEDULES for w in L.WIRES])


def _sweep(gpu, family, schedule, wire):
    cs = L.cases(family)
    assert cs
    failed = []
    for case in cs:   # (every case runs; the message names each one that failed, the first in full)
        try:
            L.run_case(gpu, case, schedule, wire)
        except AssertionError as e:
            failed.append("%s: %s" % (case.name, str(e)[:600]))
    assert not failed, "%d of %d cases of family %s failed on %s / %s:\n%s" % (len(failed), len(cs), family, schedule, wire, "\n".join(failed))


@grid
def test_family_a_read_state_machine(gpu, schedule, wire):
    _sweep(gpu, "A", schedule, wire)


@grid
def test_family_b_prefix_region_and_look_back(gpu, schedule, wire):
    _sweep(gpu, "B", schedule, wire)


@grid
def test_family_c_period(gpu, schedule, wire):
    _sweep(gpu, "C", schedule, wire)


@grid
def test_family_d_drain_size(gpu, schedule, wire):
    _sweep(gpu, "D", schedule, wire)


@grid
def test_family_d2_drain_size_with_two_sends_per_round(gpu, schedule, wire):
    _sweep(gpu, "D2", schedule, wire)


@grid
def test_family_e_ring_end(gpu, schedule, wire):
    _sweep(gpu, "E", schedule, wire)


@grid
def test_family_f_credit_threshold(gpu, schedule, wire):
    _sweep(gpu, "F", schedule, wire)


@grid
def test_family_g_table_cache_and_stale_state(gpu, schedule, wire):
    _sweep(gpu, "G", schedule, wire)


@grid
def test_family_h_tiles(gpu, schedule, wire):
    _sweep(gpu, "H", schedule, wire)


@grid
def test_family_i_no_period(gpu, schedule, wire):
    _sweep(gpu, "I", schedule, wire)


@grid
def test_family_j_send_pricing(gpu, schedule, wire):
    _sweep(gpu, "J", schedule, wire)


@pytest.mark.parametrize("wire", L.WIRES)
def test_family_g_across_a_pair_pool_recycle(gpu, wire):
    L.run_pool_recycle(gpu, wire)
