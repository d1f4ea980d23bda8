"""The body-tier scenarios on the golden model (CPU).  The model has no tiers, and none is needed:
where a body lives must be invisible to clients, so tests/tier_scenarios.py's tier operations are
left out here and each scenario is judged by ``tier_scenarios.CHECKS`` -- what the clients must
see, from the protocol.  tests/test_gpu_tier_edges.py runs the same steps with the tier
operations on the HIP data plane and holds it to the same statements, to this run's bytes and to
the device-state expectations the scenarios carry."""

import pytest

pytest.register_assert_rewrite("get_scenarios", "tier_scenarios")   # (their checks report what they compared)

from gpu_cfg import CFG
from tier_scenarios import CHECKS, END, SCENARIOS, SPILL_LAG, Ctx, RingModel, golden_plane, run_tier


@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_tier_edges(name):
    sc = SCENARIOS[name]
    g = golden_plane(dict(CFG, **sc.cfg))
    ctx = Ctx(g)
    outs = run_tier(g, sc.fn(g, ctx), ctx, sc.now_step_ms)
    CHECKS[name](outs)
    assert outs[-1]["live"] == (0, 0), "messages are still held after everything was settled"


def test_every_scenario_has_a_check():
    assert sorted(CHECKS) == sorted(SCENARIOS) == sorted(END)


def test_ring_replica_pads_to_the_wrap_and_lags_the_tail():
    """The replica itself, on a ring of 4 blocks of 100 bytes: a slot that would cross the ring's
    end starts at the wrap; the ring is full against the lowest tail of the last SPILL_LAG steps;
    the tail never enters the head's block."""
    r = RingModel(size=400, block=100, lag=SPILL_LAG)
    assert [r.reserve(90) for _ in range(4)] == [0, 90, 180, 270] and r.reserve(90) is None   # 360 + 90 > 400: padded, full
    for p in (0, 90, 180, 270):
        r.release(p, 90)
    r.end_step()
    assert r.tail == 300 and r.live == [0, 0, 0, 0]          # head 360 is in block 3: the tail stops there
    for _ in range(SPILL_LAG - 1):
        assert r.reserve(90) is None                         # an older step's tail (0) still counts
        r.end_step()
    assert r.reserve(90) == 400 and r.head == 490            # padded past the ring's end
