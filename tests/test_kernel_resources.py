"""What the planner pair's kernel may cost the launcher: no scratch segment.

k_plan_pair_mw holds five bodies (two drain planners, two send planners, the wire mover) at one wave per SIMD and the full
register file; round 6 met a version of it whose drain body indexed a register array through a loop variable -- 72 bytes of
scratch per lane -- and every launch of the kernel paid 1-2 us for it (the reference-default-knob leg 68 -> 59 GiB/s,
DESIGN.md section 2.7).  The compiler says what it allocated (tests/kernel_resources.py); this pins it."""
from tests.kernel_resources import needs_hipcc, report

pytestmark = needs_hipcc


def test_the_planner_pairs_kernel_has_no_scratch_segment():
    seen = report("grdma_rx_plan.hip")
    assert "k_plan_pair_mw" in seen, "no resource remarks for k_plan_pair_mw"
    got = seen["k_plan_pair_mw"]
    print(got)
    assert got["scratch"] == 0, got
    assert got["vspill"] == 0, got
    assert got["lds"] <= 160 * 1024, got
