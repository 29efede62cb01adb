"""The by-rule subset of the planner sweep that tests/test_planner_sweep_emu.py runs under the wave emulator, one test per
case (planner_sweep_lib.emu_subset).  Not collected by name: the hardware suite runs every case of
tests/test_zz_gpu_planner_sweep.py and needs none of them twice."""
import pytest

from tests import planner_sweep_lib as L

pytestmark = pytest.mark.gpu

SUBSET = L.emu_subset()


@pytest.mark.parametrize("entry", SUBSET, ids=["%s-%s-%s-%s" % e for e in SUBSET])
def test_case(gpu, entry):
    family, name, schedule, wire = entry
    case = next(c for c in L.cases(family) if c.name == name)
    L.check_witnesses(case)
    L.run_case(gpu, case, schedule, wire)
