"""Queue byte limits on the HIP data plane: k_byte_room, the BL instantiations of k_ring_plan /
k_enqueue / k_dequeue (trim_head's byte rule, the ready-bytes bookkeeping of every walk) and
k_basic_get in csrc/kernels/dataplane.hip.  Every scenario of tests/bytelimit_scenarios.py, in
the captured graph and with eager launches, at the default q_max and at q_max = 4096 (the two
pair-key widths), judged by the scenarios' own record and then compared step by step with the
golden model: egress bytes, counters, queue depths, ready bytes and store records must be equal."""

import pytest
import torch  # noqa: F401  (loaded before the extension initialises HIP: torch's own lazy
#                            init finds no device afterwards, and the sharded cases need it)

from bytelimit_scenarios import (OFF, SCENARIOS, WIDTHS, cfg_of, check, golden_plane, gpu_plane, run_bytes, sharded_check,
                                 sharded_cluster, sharded_run, x_death_reasons)
from e2e_scenarios import assert_same
from gpu_cfg import CFG
from route_scenarios import check_drained

pytestmark = pytest.mark.gpu

MODES = {"graph": True, "eager": False}
_golden = {}


def golden_outs(sc, key, cfg, on=True):
    """The golden model's run of a scenario: computed once, only read by the cases."""
    if key not in _golden:
        g = golden_plane(cfg, on)
        _golden[key] = run_bytes(g, sc.fn(g))
    return _golden[key]


def judge(sc, key, mode, width, on=True):
    cfg = dict(cfg_of(sc, CFG), **WIDTHS[width])
    d = gpu_plane(cfg, MODES[mode], on)
    assert d.info["queue_limits"] == 1 and d.info["queue_limit_bytes"] == int(on)
    rec = sc.fn(d)
    od = run_bytes(d, rec)
    check(rec, od)
    og = golden_outs(sc, (key, width), cfg, on)
    assert_same(og, od)
    for k, (a, b) in enumerate(zip(og, od)):
        assert a["counters"] == b["counters"], f"step {k}"
        assert a["depth"] == b["depth"], f"step {k}"
        assert a.get("bytes") == b.get("bytes"), f"step {k}: ready bytes differ"
        assert a["cap"] == b["cap"], f"step {k}: ring capacities differ"
        assert a.get("consumed") == b.get("consumed"), f"step {k}: store records differ"
    if sc.drained:
        check_drained(d.last_counters, cfg["log_block"])
        assert all(d.message_count(q.slot) == 0 for q in d.queues.values())
        if on:
            assert all(d.queue_bytes(q.slot) == 0 for q in d.queues.values())
    if sc.cfg.get("x_death"):
        assert x_death_reasons(od, 2, 1) == ["maxlen"] * len(rec.died)
    return d


@pytest.mark.parametrize("width", sorted(WIDTHS))
@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_bytelimits(gpu, name, mode, width):
    judge(SCENARIOS[name], name, mode, width)


@pytest.mark.parametrize("mode", sorted(MODES))
def test_off_is_today(gpu, mode):
    """``queue_limits`` on, the byte flag off: the keyword is ignored and ``info`` reports 0."""
    judge(OFF, "off", mode, "narrow", on=False)


@pytest.mark.parametrize("lag", [0, 1])
def test_sharded_owner_enforces(gpu, lag):
    """Byte-limited queues owned by rank 1, published from rank 0: the owner trims or refuses, the
    publisher gets Acks, and the outputs equal the golden cluster's."""
    key = ("sharded", lag)
    if key not in _golden:
        _golden[key] = sharded_run(sharded_cluster(CFG, lag))
    outs = sharded_run(sharded_cluster(CFG, lag, gpu=True))
    sharded_check(outs)
    assert outs == _golden[key]
