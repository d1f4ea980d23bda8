"""Basic.Get between steps on the golden model (CPU): every scenario of tests/get_scenarios.py,
judged by ``get_scenarios.CHECKS`` -- what the protocol says the clients must see, decoded from
the Gets' frames, never taken from the model.  tests/test_gpu_get_edges.py holds the HIP data
plane (k_basic_get) to the same statements and to byte equality with this model."""

import pytest

pytest.register_assert_rewrite("get_scenarios", "tier_scenarios")   # (their checks report what they compared)

from get_scenarios import CHECKS, SCENARIOS, golden_plane, run_get
from gpu_cfg import CFG


def run_golden(sc):
    g = golden_plane(dict(CFG, **sc.cfg))
    return g, run_get(g, sc.fn(g), sc.now_step_ms)


@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_get_edges(name):
    g, outs = run_golden(SCENARIOS[name])
    CHECKS[name](outs)
    if not name.startswith(("window_noack", "frame_split")):   # (those leave messages queued or unsettled)
        assert outs[-1]["live"] == (0, 0), "a message is still held after everything was settled"


def test_every_scenario_has_a_check():
    assert sorted(CHECKS) == sorted(SCENARIOS)
