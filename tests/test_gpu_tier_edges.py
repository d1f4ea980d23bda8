"""The body tiers on the HIP data plane: every scenario of tests/tier_scenarios.py with its tier
operations applied (k_spill / spill_queue, stage_spill inside k_dequeue, spill_reserve, the
ring's tail in final_step, k_cold_pick / k_cold_commit / k_cold_scan / k_cold_in and the
q_cold_lim holds), on a small plane of its own -- log_block 64 KiB, a 1 MiB log, a 512 KiB spill
ring, a ColdStore under tmp_path -- in the captured graph and with eager launches.

Each run is judged three ways: by the scenario's client-side ``CHECKS`` (the protocol), against
the golden model's run of the same steps without the tier operations (step by step where the
scenario pages cold bodies in before they are due, else by what each connection saw over the
whole run), and by the device-state expectations the scenario carries (bytes moved, live bytes
per tier, q_cold_lim, the ring against its replica).  Then the end state: after everything is
consumed and SPILL_LAG + 1 empty steps no message and no byte is live in any tier, the ring's
tail is within a block of its head, and the store's gc unlinks every segment but the current."""

import pytest
import torch  # noqa: F401  (loaded before the extension initialises HIP)

pytest.register_assert_rewrite("get_scenarios", "tier_scenarios")   # (their checks report what they compared)

from e2e_scenarios import assert_same
from get_scenarios import gpu_plane
from gpu_cfg import CFG
from tier_scenarios import (CHECKS, END, SCENARIOS, TIER, Ctx, assert_end_state, dev, golden_plane, run_tier,
                            seen_by_conn)

pytestmark = pytest.mark.gpu

MODES = {"graph": True, "eager": False}
_golden = {}


def golden_outs(name):
    """The golden model's run of a scenario: computed once, only read by the cases."""
    if name not in _golden:
        sc = SCENARIOS[name]
        g = golden_plane(dict(CFG, **sc.cfg))
        ctx = Ctx(g)
        _golden[name] = run_tier(g, sc.fn(g, ctx), ctx, sc.now_step_ms)
    return _golden[name]


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_tier_edges(gpu, tmp_path, name, mode):
    from chanamq_amd.store.cold import ColdStore
    sc = SCENARIOS[name]
    d = gpu_plane(dict(CFG, **sc.cfg), MODES[mode], **sc.kw)
    # (log_block is not in info(): the ring's live bytes are kept per block)
    assert (d.info["log_bytes"], d.info["spill_bytes"], len(dev(d, "spill_live"))) == (
        TIER["log_bytes"], TIER["spill_bytes"], TIER["spill_bytes"] // TIER["log_block"]), "not the tier configuration asked for"
    store = ColdStore(str(tmp_path / "cold"))
    try:
        ctx = Ctx(d, store)
        od = run_tier(d, sc.fn(d, ctx), ctx, sc.now_step_ms)
        CHECKS[name](od)                    # what the clients must see, from the protocol
        og = golden_outs(name)
        if sc.lockstep:
            assert_same(og, od)             # the model's bytes, step by step
            for k, (a, b) in enumerate(zip(og, od)):
                assert a["counters"] == b["counters"], f"step {k}: golden {a['counters']}, engine {b['counters']}"
                assert a["after"] == b["after"], f"step {k}: golden {a['after']}, engine {b['after']}"
        else:
            assert seen_by_conn(og) == seen_by_conn(od)
            assert og[-1]["after"] == od[-1]["after"]
        assert_end_state(d, ctx, END[name])
    finally:
        store.close()
