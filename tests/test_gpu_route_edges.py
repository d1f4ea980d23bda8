"""The middle of the step on the HIP data plane -- k_route (topic_group / topic_tile,
route_one, route_emit), k_scan_route's log_reserve, k_route_store (route_one<1>,
live_add_blocks, store_one_pre) and both enqueue paths (k_rs_hist_plan / k_rs_scatter_enq;
k_rs_hist / k_rs_scatter / k_qfirst / k_ring_plan / k_enqueue) -- at the places where those
kernels change path: every scenario of tests/route_scenarios.py, in the captured graph and
with eager launches, judged by ``route_scenarios.check_run`` (what every consumer and every
publisher must see, from the topology and the scenario's own brute-force matcher) and, where
the scenario is exact, compared byte by byte, step by step, counters included, with the
golden model.  The capacity scenarios (a full pair table, message table or body log) and an
exhausted ring pool have no golden model: their checks state what a client sees.  The sort
and enqueue group runs once per pair-key width: 8, 9, 10 and 11 bits on the fused path, two
and three 8-bit passes on the other."""

import pytest

from e2e_scenarios import assert_same
from gpu_cfg import CFG
from route_scenarios import (KEY_WIDTHS, SCENARIOS, SHARED, SORTING, check_drained, check_run, golden_plane, limits,
                             run_route)

pytestmark = pytest.mark.gpu

MODES = {"graph": True, "eager": False}
_golden = {}


def golden_outs(sc, key, cfg):
    """The golden model's run of a scenario: computed once, only read by the cases."""
    if key not in _golden:
        g = golden_plane(cfg)
        _golden[key] = run_route(g, sc.fn(g, limits()).steps, sc.now_step_ms)
    return _golden[key]


def judge(sc, key, mode, **over):
    from chanamq_amd.engine.dataplane import GpuDataPlane
    cfg = dict(CFG, **sc.cfg, **over)
    d = GpuDataPlane(graph=MODES[mode], **cfg)
    run = sc.fn(d, limits())
    od = run_route(d, run.steps, sc.now_step_ms)
    check_run(run, od)                               # what the clients must see, and the named counters
    if sc.exact:
        og = golden_outs(sc, key, cfg)
        assert_same(og, od)                          # and the model's bytes
        for k, (a, b) in enumerate(zip(og, od)):
            assert [a["counters"].get(c, 0) for c in SHARED] == [b["counters"].get(c, 0) for c in SHARED], f"step {k}"
    if sc.drained:
        check_drained(d.last_counters, cfg["log_block"])
        assert all(d.message_count(q.slot) == 0 for q in d.queues.values())
    return d, run, od


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_route_edges(gpu, name, mode):
    d, run, od = judge(SCENARIOS[name], name, mode)
    if name == "log_wrap":
        # the region that would straddle the log's end starts at the end instead: the head the
        # step before reported, and the head after
        n = d.info["log_bytes"]
        for k in run.placed["skips"]:
            before, after = od[k - 1]["counters"]["log_head"], od[k]["counters"]["log_head"]
            assert before // n + 1 == after // n and before % n + after % n > n
        k = run.placed["exact"][0]
        assert od[k]["counters"]["log_head"] % n == 0


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("q_max", KEY_WIDTHS)
@pytest.mark.parametrize("name", sorted(SORTING))
def test_sort_and_enqueue_edges(gpu, name, q_max, mode):
    d, run, od = judge(SORTING[name], (name, q_max), mode, q_max=q_max)
    assert d.info["q_max"] == q_max
