"""The header encoder -- k_h2_hpenc_scan / _walk / _emit / _commit behind grdma_h2_hpenc_encode and
grdma_h2_hpenc_set_peer -- swept over header lists built from the constants it branches on, against
tests/h2_hpenc_model.HpencModel: the wire arena whole with its fill, the block-wire table, the result block, the dynamic
table and the counters, all exact.  One test per case.  Cases, witnesses and driver: tests/h2_hpenc_sweep_lib.py
(DESIGN.md 3.1h).

Every case's witness is checked from the model alone when this module is imported: a case that does not reach the edge
it is there for fails the collection, on any machine, before anything runs on a device."""
import pytest

from tests import h2_hpenc_sweep_lib as L

pytestmark = pytest.mark.gpu

L.check_cases()
IDS = [c["id"] for c in L.CASES]


@pytest.mark.parametrize("cid", IDS)
def test_case(gpu, cid):
    L.run_case(gpu, L.by_id(cid))
