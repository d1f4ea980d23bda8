"""The headers branch of route_one (csrc/kernels/dp_headers.h) on the HIP data plane: every
scenario of tests/headers_scenarios.py, in the captured graph and with eager launches, judged
by ``route_scenarios.check_run`` from the scenarios' own brute-force matcher and compared byte
by byte, step by step, with the golden model.  The branch serves k_route (pass 0),
k_route_store (pass 1, above PUB_QC queues), k_import_route (an owner's re-match) and the walk
over exchange-to-exchange edges; the step's graph keeps its launches."""

import pytest
import torch  # noqa: F401  (loaded before the extension initialises HIP: torch's own lazy
#                            init finds no device afterwards, and the sharded cases need it)

from e2e_scenarios import assert_same
from gpu_cfg import CFG
from headers_scenarios import OFF, SCENARIOS, cfg_of, golden_plane, limits
from route_scenarios import SHARED, check_drained, check_run, run_route

pytestmark = pytest.mark.gpu

MODES = {"graph": True, "eager": False}
_golden = {}


def golden_outs(sc, key, cfg, on=True):
    """The golden model's run of a scenario: computed once, only read by the cases."""
    if key not in _golden:
        g = golden_plane(cfg, headers_match=on)
        _golden[key] = run_route(g, sc.fn(g, limits() if on else None).steps, sc.now_step_ms)
    return _golden[key]


def judge(sc, key, mode, on=True):
    from chanamq_amd.engine.dataplane import GpuDataPlane
    lim = limits() if on else None
    cfg = cfg_of(sc, CFG, lim)
    d = GpuDataPlane(graph=MODES[mode], **(dict(cfg, headers_match=True) if on else cfg))
    run = sc.fn(d, lim)
    od = run_route(d, run.steps, sc.now_step_ms)
    check_run(run, od)
    og = golden_outs(sc, key, cfg, on)
    assert_same(og, od)
    for k, (a, b) in enumerate(zip(og, od)):
        assert [a["counters"].get(c, 0) for c in SHARED] == [b["counters"].get(c, 0) for c in SHARED], f"step {k}"
    if sc.drained:
        check_drained(d.last_counters, cfg["log_block"])
        assert all(d.message_count(q.slot) == 0 for q in d.queues.values())
    return d


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_headers_edges(gpu, name, mode):
    d = judge(SCENARIOS[name], name, mode)
    assert d.info["hb_pairs"] == limits().HB_PAIRS
    assert (d.info["hb_used"], d.info["hp_used"]) == d.h_used and d.h_used[0] <= d.info["hb_max"]


@pytest.mark.parametrize("mode", sorted(MODES))
def test_off_is_today(gpu, mode):
    judge(OFF, "off", mode, on=False)


@pytest.mark.parametrize("lag", [0, 1])
@pytest.mark.parametrize("world", [2, 3])
def test_sharded_owner_rematch(gpu, world, lag):
    """k_import_route: one remote queue (MF_ONEQ), one remote + one local, two remote on one
    rank (the owner's re-match from the record's own property bytes), two remote on two ranks;
    against the scenarios' matcher and byte for byte against the golden cluster."""
    from headers_scenarios import sharded_cluster, sharded_got, sharded_run
    key = ("sharded", world, lag)
    if key not in _golden:
        _golden[key] = sharded_run(sharded_cluster(CFG, world, lag))[0]
    outs, want = sharded_run(sharded_cluster(CFG, world, lag, gpu=True))
    assert sharded_got(outs) == {q: v for q, v in want.items() if v}
    assert outs == _golden[key]
