"""The send-window planner -- k_h2_sw_plan with h2sw_piece_size, h2sw_walk_piece and h2sw_emit_piece, behind
grdma_h2_sw_frame and, as k_h2_links_sw_plan / k_h2_links_sw_emit, behind grdma_h2_sw_frame_batch -- swept over message
tables built from the constants it branches on, against tests/h2_send_model.SendModel: result block, progress, slice
lengths and table, wire image, inlined-slice pointers, header-arena bytes, windows, counters and the sentinels of an
overflowing call, all exact.  One test per case and path; family 12 is the intake's grid stride, which only a device
takes.  Cases, witnesses and driver: tests/h2_send_plan_sweep_lib.py.

Every case's witness is checked from the model alone when this module is imported: a case that does not reach the edge
it is there for fails the collection, on any machine, before anything runs on a device."""
import pytest

from tests import h2_send_plan_sweep_lib as L

pytestmark = pytest.mark.gpu

L.check_cases()
TESTS = L.tests()


@pytest.mark.parametrize("cid,path", TESTS, ids=["%s-%s" % t for t in TESTS])
def test_case(gpu, cid, path):
    L.run_case(gpu, L.by_id(cid), path)
