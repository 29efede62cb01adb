"""The header decoder -- k_h2_hpack_gather / _copy / _split / _walk / _emit / _commit / _resize behind
grdma_h2_hpack_decode and grdma_h2_hpack_set_max_table_size -- swept over header blocks built from the constants it
branches on, against tests/h2_hpack_model.HpackModel: block table, field table and string arena whole with their
sentinels, the result block, the dynamic table and the counters, all exact.  One test per case.  Cases, witnesses and
driver: tests/h2_hpack_sweep_lib.py.

Every case's witness is checked from the model alone when this module is imported: a case that does not reach the edge
it is there for fails the collection, on any machine, before anything runs on a device."""
import pytest

from tests import h2_hpack_sweep_lib as L

pytestmark = pytest.mark.gpu

L.check_cases()
IDS = [c["id"] for c in L.CASES]


@pytest.mark.parametrize("cid", IDS)
def test_case(gpu, cid):
    L.run_case(gpu, L.by_id(cid))
