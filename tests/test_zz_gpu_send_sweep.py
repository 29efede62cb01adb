"""The general Send planners -- tx_plan_body (k_tx_plan: every blocking Send, and in latency mode every Send above 64 slices
or 64 KiB) and tx_burst_wave (k_tx_plan_seq: the bursts of an asynchronous endpoint on the direct wire) -- swept over slice
lists built from the constants they branch on, against the oracle: accepted bytes, work requests, ring image, staging
image, state of both sides and GetWritableSize after every Send, the delivered bytes after every drain, and on every
blocking non-latency Send the priced window the planner leaves in tx_dbg[7] against the restated pricing rule's.
One test per case and wire.  Cases, witnesses and driver: tests/send_sweep_lib.py.

Every case's witnesses are checked from the oracle alone when this module is imported: a case that does not reach the
edge it is there for fails the collection, on any machine, before anything runs on a device."""
import pytest

from tests import send_sweep_lib as L

pytestmark = pytest.mark.gpu

L.check_cases()
TESTS = L.tests()


@pytest.mark.parametrize("cid,wire", TESTS, ids=["%s-%s" % t for t in TESTS])
def test_case(gpu, cid, wire):
    L.run_case(gpu, L.by_id(cid), wire)
