"""The by-rule subset of the Send sweep that tests/test_send_sweep_emu.py runs under the wave emulator, one test per
case (send_sweep_lib.emu_subset).  Not collected by name: the hardware suite runs every case of
tests/test_zz_gpu_send_sweep.py and needs none of them twice."""
import pytest

from tests import send_sweep_lib as L

pytestmark = pytest.mark.gpu

SUBSET = L.emu_subset()


@pytest.mark.parametrize("cid,wire", SUBSET, ids=["%s-%s" % e for e in SUBSET])
def test_case(gpu, cid, wire):
    L.run_case(gpu, L.by_id(cid), wire)
