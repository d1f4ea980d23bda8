"""The ingress half of the step (k_frame_scan, and k_decode's numbering of what it emits) at
the places where the scan changes path: every scenario of tests/ingress_scenarios.py on the
HIP data plane, judged by the model-free checks of ``ingress_scenarios.check_run`` and, where
the scenario is exact, compared byte by byte, step by step, with the golden model.  Scenarios
that run into a device limit the model does not have (candidate slots, cmd_max, frag_max)
are judged by the checks alone: which segment gives way depends on the order the blocks
finish in.

Modes: the captured graph, eager launches, and ``work-copy`` (scan_in_place = 0: the fused
path that writes the work buffer and never splits) for the groups that are about where the
bytes are read from."""

import pytest

from chanamq_amd.engine.layout import SS_FRAME_ERROR, SS_TOO_LARGE
from consumer_scenarios import GOLDEN_KEYS, golden_plane, run_consumer
from dp_scenarios import NOW
from dp_scenarios import SCENARIOS as DP_SCENARIOS
from dp_scenarios import run
from e2e_scenarios import assert_same
from gpu_cfg import CFG
from ingress_scenarios import PROP_CFG, SCENARIOS, check_props, check_run, frame_max_record, limits, run_props

pytestmark = pytest.mark.gpu

MODES = {"graph": dict(graph=True), "eager": dict(graph=False), "work-copy": dict(graph=True, scan_in_place=0)}
CASES = [(name, mode) for name in sorted(SCENARIOS) for mode in sorted(MODES)
         if mode != "work-copy" or SCENARIOS[name].group in "ABC"]
_golden = {}


def golden_outs(name):
    """The golden model's run of a scenario: computed once, only read by the cases."""
    if name not in _golden:
        sc = SCENARIOS[name]
        g = golden_plane(dict(CFG, **sc.cfg))
        _golden[name] = run_consumer(g, sc.fn(g, limits()).steps)
    return _golden[name]


def gpu_run(name, mode):
    from chanamq_amd.engine.dataplane import GpuDataPlane
    sc = SCENARIOS[name]
    d = GpuDataPlane(**MODES[mode], **dict(CFG, **sc.cfg))
    r = sc.fn(d, limits())
    return d, r, run_consumer(d, r.steps)


@pytest.mark.parametrize("name,mode", CASES)
def test_ingress_edges(gpu, name, mode):
    d, r, od = gpu_run(name, mode)
    check_run(r, od)                          # what was sent must come out, from the streams alone
    if SCENARIOS[name].exact:
        assert_same(golden_outs(name), od)    # and the model's bytes
    if name.startswith("acks"):               # every delivery was acked: nothing lives, nothing waits
        assert d.last_counters["n_live_msgs"] == 0 and d.last_counters["live_bytes"] == 0
        assert all(d.message_count(q.slot) == 0 for q in d.queues.values())
    if name == "carry_too_large":
        assert (1, SS_TOO_LARGE, 0, 0) in od[0]["segs"]


@pytest.mark.parametrize("mode", sorted(MODES))
def test_frame_max_error_offset(gpu, mode):
    """The frame above the connection's frame-max: SS_FRAME_ERROR with everything before it
    consumed and err_off at the frame."""
    from chanamq_amd.engine.dataplane import GpuDataPlane
    sc = SCENARIOS["frame_max"]
    d = GpuDataPlane(**MODES[mode], **dict(CFG, **sc.cfg))
    r = sc.fn(d, limits())
    want = frame_max_record(r)
    res = d.step(r.steps[0])
    mine = [s for s in res.segs if s[0] == 1]
    assert len(mine) == 1 and tuple(mine[0][:4]) == want and want[1] == SS_FRAME_ERROR
    assert mine[0][5] == want[2], f"err_off {mine[0][5]}, the frame is at {want[2]}"


# seg_max above DEC_SEG_LDS (4096): k_decode numbers publishes and acks from the grid-wide
# rank scan over the commands instead of the frame scan's per-segment ordinals
RANK_SCAN = dict(seg_max=4097, carry_cap=1 << 16)


@pytest.mark.parametrize("mode", ["eager", "graph"])
@pytest.mark.parametrize("name", ["direct_split", "manual_ack", "mixed_multiple_settles"])
def test_rank_scan_numbering(gpu, name, mode):
    from chanamq_amd.engine.dataplane import GpuDataPlane
    cfg = dict(CFG, **RANK_SCAN)
    g = golden_plane(cfg)
    d = GpuDataPlane(**MODES[mode], **cfg)
    og = run(g, DP_SCENARIOS[name](g), now_step_ms=3000)
    od = run(d, DP_SCENARIOS[name](d), now_step_ms=3000)
    assert_same(og, od)


def golden_props():
    if "props" not in _golden:
        from chanamq_amd.engine.golden import GoldenDataPlane
        g = GoldenDataPlane(persist=True, **{k: CFG[k] for k in GOLDEN_KEYS})
        _golden["props"] = run_props(g, NOW)
    return _golden["props"]


@pytest.mark.parametrize("mode", ["eager", "graph"])
def test_property_decode(gpu, mode):
    """k_decode's property walk (a 32-byte register window, then memory reads) against the
    test's own byte-by-byte walk -- persistence, expiry and timestamp as the persist records
    of durable queues carry them, expiry also by what is still delivered later -- and against
    the golden model's records and egress."""
    from chanamq_amd.engine.dataplane import GpuDataPlane
    d = GpuDataPlane(**MODES[mode], **dict(CFG, **PROP_CFG))
    cases, records, outs = run_props(d, NOW)
    check_props(d, cases, records, outs, NOW)
    _, grecords, gouts = golden_props()
    assert sorted(r[1:] for r in records) == sorted(r[1:] for r in grecords)   # (all but the message id)
    for k, (a, b) in enumerate(zip(gouts, outs)):
        assert sorted(a["segs"]) == sorted(b["segs"]), f"step {k} segs"
        assert a["egress"] == b["egress"], f"step {k} egress"
