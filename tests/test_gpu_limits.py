"""Queue length limits on the HIP data plane: the drop-head trim of k_dequeue (trim_head in
csrc/kernels/dataplane.hip) and the reject-publish refusal of enq_store, on both enqueue paths
(k_rs_scatter_enq and k_ring_plan + k_enqueue).  Every scenario of tests/limit_scenarios.py, in
the captured graph and with eager launches, judged by the scenarios' own record and then
compared step by step with the golden model: egress bytes, counters (the two new ones
included), queue depths and store records must be equal."""

import pytest
import torch  # noqa: F401  (loaded before the extension initialises HIP: torch's own lazy
#                            init finds no device afterwards, and the sharded cases need it)

from e2e_scenarios import assert_same
from gpu_cfg import CFG
from limit_scenarios import (OFF, SCENARIOS, cfg_of, check, golden_plane, gpu_plane, run_limits, sharded_check,
                             sharded_cluster, sharded_run)
from route_scenarios import check_drained

pytestmark = pytest.mark.gpu

MODES = {"graph": True, "eager": False}
_golden = {}


def golden_outs(sc, key, cfg, on=True):
    """The golden model's run of a scenario: computed once, only read by the cases."""
    if key not in _golden:
        g = golden_plane(cfg, on)
        _golden[key] = run_limits(g, sc.fn(g))
    return _golden[key]


def judge(sc, key, mode, on=True):
    cfg = cfg_of(sc, CFG)
    d = gpu_plane(cfg, MODES[mode], on)
    assert d.info["queue_limits"] == int(on)
    rec = sc.fn(d)
    od = run_limits(d, rec)
    check(rec, od)
    og = golden_outs(sc, key, cfg, on)
    assert_same(og, od)
    for k, (a, b) in enumerate(zip(og, od)):
        assert a["counters"] == b["counters"], f"step {k}"
        assert a["depth"] == b["depth"], f"step {k}"
        assert a.get("consumed") == b.get("consumed"), f"step {k}: store records differ"
    if sc.drained:
        check_drained(d.last_counters, cfg["log_block"])
        assert all(d.message_count(q.slot) == 0 for q in d.queues.values())
    return d


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_limits(gpu, name, mode):
    judge(SCENARIOS[name], name, mode)


@pytest.mark.parametrize("mode", sorted(MODES))
def test_off_is_today(gpu, mode):
    judge(OFF, "off", mode, on=False)


@pytest.mark.parametrize("lag", [0, 1])
def test_sharded_owner_enforces(gpu, lag):
    """A limited queue owned by rank 1, published from rank 0: the owner trims or refuses, the
    publisher gets Acks, and the outputs equal the golden cluster's."""
    key = ("sharded", lag)
    if key not in _golden:
        _golden[key] = sharded_run(sharded_cluster(CFG, lag))
    outs = sharded_run(sharded_cluster(CFG, lag, gpu=True))
    sharded_check(outs)
    assert outs == _golden[key]
