"""x-death headers and cycle detection on the HIP data plane: the size pass (k_dead_size), the
rewrite in phase 1 of k_dead_pack<true> and the ban check of the dead view's routing
(csrc/kernels/dp_xdeath.h, xdeath_plan.h, dataplane.hip, engine.hip launch_dead).  Every scenario of
tests/xdeath_scenarios.py, in the captured graph and with eager launches, judged by the scenarios'
own record -- property bytes included -- and then compared step by step with the golden model:
egress bytes, counters (n_dl_cycle included), queue depths and store records must be equal."""

import pytest
import torch  # noqa: F401  (loaded before the extension initialises HIP)

from e2e_scenarios import assert_same
from gpu_cfg import CFG
from route_scenarios import check_drained
from xdeath_scenarios import SCENARIOS, check, golden_plane, gpu_plane, run_xd

pytestmark = pytest.mark.gpu

MODES = {"graph": True, "eager": False}
_golden = {}


def golden_outs(sc, key, cfg):
    """The golden model's run of a scenario: computed once, only read by the cases."""
    if key not in _golden:
        g = golden_plane(cfg)
        _golden[key] = run_xd(g, sc.fn(g))
    return _golden[key]


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_xdeath(gpu, name, mode):
    sc = SCENARIOS[name]
    cfg = dict(CFG, **sc.cfg)
    d = gpu_plane(cfg, MODES[mode])
    assert d.info["dead_letter"] == 1 and d.info["x_death"] == 1
    rec = sc.fn(d)
    od = run_xd(d, rec)
    check(rec, od)
    og = golden_outs(sc, name, cfg)
    assert_same(og, od)
    for k, (a, b) in enumerate(zip(og, od)):
        assert a["counters"] == b["counters"], f"step {k}"
        assert a["depth"] == b["depth"], f"step {k}"
        assert a.get("consumed") == b.get("consumed"), f"step {k}: store records differ"
        assert a.get("stored") == b.get("stored"), f"step {k}: persist records differ"
    if sc.drained:   # every reference is dropped: refused pairs took none
        check_drained(d.last_counters, cfg["log_block"])
        assert all(d.message_count(q.slot) == 0 for q in d.queues.values())


def test_x_death_needs_dead_letter():
    from chanamq_amd.engine.dataplane import GpuDataPlane
    with pytest.raises(ValueError, match="dead_letter"):
        GpuDataPlane(x_death=True, **CFG)
