"""The back of the step on the HIP data plane -- k_dv_write, k_conn_layout and its twin
k_conn_sizes / k_scan / k_conn_out, set_egress_bytes and the gather table, k_render
(render_return, render_confirms, render_deliv), k_post's tag hand-over, k_persist_size and
k_persist_pack -- at the places where those kernels change path: every scenario of
tests/egress_scenarios.py, in the captured graph and with eager launches.  A run is judged
first by ``egress_scenarios.check_run`` -- the bytes every connection must receive, rendered
by the scenario's own record with the host codec, the frames walked on their own, and the
counters only this plane keeps (run count, returns, confirm frames, referenced deliveries and
their bytes, live messages) -- and then compared byte by byte, step by step, with the golden
model."""

import pytest

from e2e_scenarios import assert_same
from egress_scenarios import (PERSIST, SCENARIOS, SHARED, WIDE, WIDE_BASE, check_drained, check_persist, check_run, env_of,
                              golden_plane, limits, run_egress, same_copies, wide_cfg)
from gpu_cfg import CFG

pytestmark = pytest.mark.gpu

MODES = {"graph": True, "eager": False}
_golden, _gpu = {}, {}


def golden_outs(sc, key, cfg):
    """The golden model's run of a scenario: computed once, only read by the cases."""
    if key not in _golden:
        g = golden_plane(cfg)
        _golden[key] = run_egress(g, sc.fn(g, limits(), env_of(g, cfg)).steps, persist=bool(cfg.get("persist")))
    return _golden[key]


def judge(sc, key, mode, cfg=None):
    """One run on the HIP plane (kept per scenario and mode: the comparisons between two
    scenarios read it again), through the checks and against the model."""
    from chanamq_amd.engine.dataplane import GpuDataPlane
    if (key, mode) in _gpu:
        return _gpu[(key, mode)]
    cfg = dict(CFG, **(sc.cfg if cfg is None else cfg))
    d = GpuDataPlane(graph=MODES[mode], **cfg)
    run = sc.fn(d, limits(), env_of(d, cfg))
    od = run_egress(d, run.steps, persist=bool(cfg.get("persist")))
    check_run(run, od)
    og = golden_outs(sc, (sc.fn, cfg["c_max"]), cfg)      # (the model's run does not depend on egress by reference)
    assert_same(og, od)
    for k, (a, b) in enumerate(zip(og, od)):
        assert [a["counters"].get(c, 0) for c in SHARED] == [b["counters"].get(c, 0) for c in SHARED], f"step {k}"
    run.net.dp = None                # (the engine goes; the record and the outputs stay)
    _gpu[(key, mode)] = (d.info, run, od)
    return _gpu[(key, mode)]


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_egress_edges(gpu, name, mode):
    info, run, od = judge(SCENARIOS[name], name, mode)
    if name in ("runs_lds", "deliv_passes", "mixed_channel", "deliver_fields", "ref_edges", "cap_regions"):
        check_drained(od)
    if name == "runs_lds":       # the step's run count, as k_dv_write read it
        assert [o["counters"]["n_runs"] for o in od[:3]] == run.placed["runs"] == [limits().DVW_LDS + k for k in (-1, 0, 1)]
    if name.startswith("ref_edges"):
        assert (od[0]["counters"]["n_ref"] > 0) == (name == "ref_edges")


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("name", ["deliv_passes", "ref_edges"])
def test_spliced_egress_is_the_inline_rendering(gpu, name, mode):
    """Egress by reference against ``egress_ref=None``: the bytes on the wire are the same."""
    _, _, by_ref = judge(SCENARIOS[name], name, mode)
    _, _, inline = judge(SCENARIOS[name + "_inline"], name + "_inline", mode)
    assert all(o["counters"]["n_ref"] == 0 for o in inline)
    assert [o["egress"] for o in by_ref] == [o["egress"] for o in inline]


@pytest.mark.parametrize("mode", sorted(MODES))
def test_conn_wide(gpu, mode):
    """c_max CONN_LAYOUT_MAX + 2: k_conn_sizes, the scan and k_conn_out lay the connections
    out.  Through the checks and against the model, and every four-region connection gets the
    bytes the same traffic gives it on the single-block path."""
    lim = limits()
    info, wide, ow = judge(WIDE, "conn_wide", mode, wide_cfg(lim))
    assert info["c_max"] == lim.CONN_LAYOUT_MAX + 2 > lim.CONN_LAYOUT_MAX
    _, base, ob = judge(WIDE_BASE, "conn_wide_base", mode)
    same_copies(wide, ow, base, ob)


@pytest.mark.parametrize("mode", sorted(MODES))
def test_persist_pack(gpu, mode):
    """What k_persist_pack writes: parsed, against the scenario's own expectation and the
    model's records; the packed buffer's sizes and offsets walked on their own."""
    info, run, od = judge(PERSIST, "persist_pack", mode)
    check_persist(run, od, raw=True)
    og = golden_outs(PERSIST, (PERSIST.fn, CFG["c_max"]), dict(CFG, **PERSIST.cfg))
    for k, (a, b) in enumerate(zip(og, od)):     # (all but the message id)
        assert sorted(r[1:] for r in a["persist"]) == sorted(r[1:] for r in b["persist"]), f"step {k}"
    assert sum(len(o["persist"]) for o in od) == run.placed["records"] and run.placed["stored"] > info["msg_max"]


def test_egress_buffer_holds_the_worst_step(gpu):
    """The egress buffer against what one step can render: deliveries and GetEmpty frames up
    to egress_cap (the dequeue's byte budget), every publish of a full work buffer returned
    with the longer reply text (72 bytes each over what it took in the work buffer), a confirm
    frame on every channel, and the gather table behind the rendered bytes."""
    from chanamq_amd.engine.dataplane import GpuDataPlane
    i = GpuDataPlane(graph=False, **CFG).info
    worst = (i["egress_cap"] + i["work_cap"] + 72 * i["pub_max"] + 21 * i["c_max"] * i["chpc"] + 15 + 16 * i["deliv_max"])
    assert i["pub_max"] == CFG["cmd_max"] and 72 * i["pub_max"] > 4096
    assert i["egress_alloc"] >= worst, (i["egress_alloc"], worst)


def test_egress_buffer_past_4g_is_refused(gpu):
    """ConnOut.off and EgressRef.dst are 32-bit: a config whose egress buffer would pass
    4 GiB is refused by the constructor's sizing checks, before anything is allocated."""
    from chanamq_amd.engine.dataplane import GpuDataPlane
    i = GpuDataPlane(graph=False, **CFG).info
    fixed = i["egress_alloc"] - i["egress_cap"]
    with pytest.raises(RuntimeError, match="egress buffer must stay below 4 GiB"):
        GpuDataPlane(graph=False, **dict(CFG, egress_cap=(4 << 30) - fixed))
