"""The many-link header encoder -- k_h2_links_hpenc_scan / _walk / _emit / _commit behind grdma_h2_hpenc_encode_batch --
over the cases of the single encoder's sweep (tests/h2_hpenc_sweep_lib.py): every case of a family is a
link of its own, and step k of every case that has a step k is ONE batch call (at most 256 links a call; a case's
("peer", ...) steps are applied on the host in between).  Every link is compared with its own model as a single call is:
the whole wire arena, the block-wire table, the result tuple, the table dump and the counters, all exact.  Of family 4
the cases sized for a link's share of the grid (4 x 256 lanes) run here."""
import pytest

from tests import h2_hpenc_sweep_lib as L

pytestmark = pytest.mark.gpu

L.check_cases()


@pytest.mark.parametrize("fam", L.FAMILIES)
def test_family(gpu, fam):
    assert L.links_cases(fam)
    L.run_links(gpu, fam)
