"""Dead-lettering on the HIP data plane: the dead list (dead_leave in k_dequeue's TTL walk and
trim_head, US_DEAD in k_chan_advance), k_dead_pack and the dead pass through the import path
(csrc/kernels/dataplane.hip, engine.hip launch_dead).  Every scenario of tests/dlx_scenarios.py,
in the captured graph and with eager launches, judged by the scenarios' own record and then
compared step by step with the golden model: egress bytes, counters (the new ones included),
queue depths and store records must be equal."""

import pytest
import torch  # noqa: F401  (loaded before the extension initialises HIP)

from dlx_scenarios import OFF, SCENARIOS, cfg_of, check, golden_plane, gpu_plane, run_dlx
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
        _golden[key] = run_dlx(g, sc.fn(g, on))
    return _golden[key]


def judge(sc, key, mode, on=True):
    cfg = cfg_of(sc, CFG)
    d = gpu_plane(cfg, MODES[mode], on)
    assert d.info["dead_letter"] == int(on)
    rec = sc.fn(d, on)
    od = run_dlx(d, rec)
    check(rec, od)
    og = golden_outs(sc, (key, on), cfg, on)
    assert_same(og, od)
    for k, (a, b) in enumerate(zip(og, od)):
        assert a["counters"] == b["counters"], f"step {k}"
        assert a["depth"] == b["depth"], f"step {k}"
        assert a.get("consumed") == b.get("consumed"), f"step {k}: store records differ"
        assert a.get("stored") == b.get("stored"), f"step {k}: persist records differ"
    if sc.drained and on:
        check_drained(d.last_counters, cfg["log_block"])
        assert all(d.message_count(q.slot) == 0 for q in d.queues.values())
    return d


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_dlx(gpu, name, mode):
    judge(SCENARIOS[name], name, mode)


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("name", ["ttl_edges", "rejects", "routing"])
def test_off_ignores_the_arguments(gpu, name, mode):
    judge(SCENARIOS[name], name, mode, on=False)


@pytest.mark.parametrize("mode", sorted(MODES))
def test_off_is_today(gpu, mode):
    judge(OFF, "off", mode, on=False)


def test_spilled_body(gpu):
    """A body that lies in the host spill ring (SPILL_BIT) when its entry dies is copied from
    there: the dead letter carries it verbatim."""
    from chanamq_amd.engine.traffic import publish_command
    from dlx_scenarios import NOW, VH, observe
    cfg = dict(CFG, spill_bytes=8 << 20)
    d = gpu_plane(cfg, True)
    d.declare_exchange(VH, "dlx", "fanout")
    d.declare_queue(VH, "park")
    d.bind(VH, "park", "dlx", "")
    d.declare_queue(VH, "src", dead_letter_exchange="dlx")
    d.open_connection(1, VH)
    d.open_channel(1, 1)
    d.open_connection(2, VH)
    d.open_channel(2, 1)
    bodies = [bytes((i + k) & 255 for i in range(3000 + k)) for k in range(4)]
    d.step({1: b"".join(publish_command(1, "", "src", b, {"expiration": "1000"}) for b in bodies)}, now_ms=NOW)
    assert d.spill(frac=1.0, hot=0) > 0
    d.step({}, now_ms=NOW + 2000)
    assert d.last_counters["n_dl_expired"] == 4
    d.consume(2, 1, VH, "park", "c", no_ack=True)
    r = d.step({}, now_ms=NOW + 2001)
    ev = observe(dict(egress=r.egress), 2)
    assert [e[4] for e in ev[(2, 1)]] == bodies and all(e[1] == "dlx" and e[2] == b"src" for e in ev[(2, 1)])


def test_sharded_plane_is_refused():
    from chanamq_amd.engine.dataplane import GpuDataPlane
    with pytest.raises(ValueError, match="sharded"):
        GpuDataPlane(dead_letter=True, world=2, rank=0, **CFG)
