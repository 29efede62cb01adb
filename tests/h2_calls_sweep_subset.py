"""The subset of the call table's sweep that tests/test_h2_calls_sweep_emu.py runs under the wave emulator, one test per
case (h2_calls_sweep_lib.emu_subset).  Not collected by name: the hardware suite runs every case of
tests/test_zz_gpu_h2_calls_sweep.py and needs none of them twice."""
import pytest

from tests import h2_calls_sweep_lib as L

pytestmark = pytest.mark.gpu

SUBSET = L.emu_subset()


@pytest.mark.parametrize("cid", SUBSET)
def test_case(gpu, cid):
    L.run_case(gpu, L.by_id(cid))
