"""GPU: the latency engine's one-wave send and drain at their edges.

rxw_fast (the watcher's single-wave drain), the unary branch of tx_small_wave and the Send straight from the doorbell
wave, on message sequences built from the constants they branch on (tests/latency_sweep_lib.py): one connection a -> b,
b's reads carried out by a watcher, every drain's endpoint reads and would_block compared with the oracle's as they
come; behind the sequence the number of single-wave drains EQUAL to what a plain Python restatement of rxw_fast's and
express_fits' guards predicts from oracle state alone (a drain that wrongly declines is delivered by the plan body with
the same bytes), watch_hits, every state field of both ends, leftover_cap, both ring images and the contents of b's
record-size history.  Every case with GRDMA_WATCH_FAST 1 and 0 (0: predicted count 0, same bytes).

The send side has no counter (one would sit on the round trip's path): family F is parity -- bytes, state, rings,
history -- under both settings of GRDMA_ENGINE_DIRECT_SEND, with the receiver's count still exact; the Send that the
free space cuts is parity only, its drain count included.  Family G (ordered wire) predicts 0.

The witnesses of every case are checked when this module is imported, on any machine: a case that does not reach its
edge fails collection.  Runs under the emulator too (tests/test_emu_gpu_suite.py)."""
import pytest

from tests import latency_sweep_lib as L

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300, method="thread")]

CASES = L.check_cases()
RECEIVE = [c for c in CASES if c["fam"] != "F"]
SEND = [c for c in CASES if c["fam"] == "F"]


@pytest.mark.parametrize("fast", ["1", "0"], ids=["single_wave_drain", "plan_body_only"])
@pytest.mark.parametrize("c", RECEIVE, ids=[c["id"] for c in RECEIVE])
def test_drains_at_the_edges_of_the_single_wave_path(gpu, c, fast, monkeypatch):
    monkeypatch.setenv("GRDMA_WATCH_FAST", fast)
    monkeypatch.delenv("GRDMA_ENGINE_DIRECT_SEND", raising=False)
    L.run_on_device(gpu, c["seq"], fast == "1", c["exact"])


@pytest.mark.parametrize("fast", ["1", "0"], ids=["single_wave_drain", "plan_body_only"])
@pytest.mark.parametrize("direct", [None, "0"], ids=["send_from_the_doorbell_wave", "send_through_the_workgroup"])
@pytest.mark.parametrize("c", SEND, ids=[c["id"] for c in SEND])
def test_sends_at_the_edges_of_the_unary_branch_and_the_fast_lane(gpu, c, direct, fast, monkeypatch):
    """Parity only on the send side: there is no counter that says which way a Send took."""
    monkeypatch.setenv("GRDMA_WATCH_FAST", fast)
    if direct is None:
        monkeypatch.delenv("GRDMA_ENGINE_DIRECT_SEND", raising=False)
    else:
        monkeypatch.setenv("GRDMA_ENGINE_DIRECT_SEND", direct)
    L.run_on_device(gpu, c["seq"], fast == "1", c["exact"])
