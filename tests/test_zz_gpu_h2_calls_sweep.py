"""The call table -- the eight k_h2_calls_* kernels behind grdma_h2_calls_step -- swept over tables built from the
constants its stages branch on, against tests/h2_calls_model.CallsModel: the dispatch table, the segment words and the
done list whole with their fill, the result block, the dump and the counters, all exact.  One test per case.  Cases,
witnesses and driver: tests/h2_calls_sweep_lib.py.

Every case's witness is checked from the model alone when this module is imported: a case that does not reach the edge
it is there for fails the collection, on any machine, before anything runs on a device."""
import pytest

from tests import h2_calls_sweep_lib as L

pytestmark = pytest.mark.gpu

L.check_cases()
IDS = [c["id"] for c in L.CASES]


@pytest.mark.parametrize("cid", IDS)
def test_case(gpu, cid):
    L.run_case(gpu, L.by_id(cid))
