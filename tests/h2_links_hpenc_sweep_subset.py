"""What tests/test_h2_links_hpenc_sweep_emu.py runs under the wave emulator: the families of
tests/test_zz_gpu_h2_links_hpenc_sweep.py through the batch call, each cut down to its cases of the by-rule subset
(h2_hpenc_sweep_lib.emu_subset).  Not collected by name."""
import pytest

from tests import h2_hpenc_sweep_lib as L

pytestmark = pytest.mark.gpu

SUBSET = set(L.emu_subset())


@pytest.mark.parametrize("fam", L.FAMILIES)
def test_family(gpu, fam):
    assert [c for c in L.links_cases(fam) if c["id"] in SUBSET]
    L.run_links(gpu, fam, only=SUBSET)
