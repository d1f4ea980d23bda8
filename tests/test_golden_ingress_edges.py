"""The ingress-half scenarios on the golden model (CPU), judged by the model-free checks of
``ingress_scenarios``: what every consumer must receive, that every segment record accounts
for its bytes, the kick rule, and that every scenario is done after its fixed number of empty
steps.  The model never runs out of candidate slots or step capacity, so it passes them with
room to spare; this proves the inputs are within the checks under the reference alone, and
holds the model to them.  tests/test_gpu_ingress_edges.py holds the HIP data plane to the
same checks and, where a scenario is marked exact, to byte equality with this model."""

import pytest

from chanamq_amd.engine.layout import SS_TOO_LARGE
from consumer_scenarios import GOLDEN_KEYS, golden_plane, run_consumer
from dp_scenarios import NOW
from gpu_cfg import CFG
from ingress_scenarios import (EXPIRATIONS, SCENARIOS, check_props, check_run, commands, frame_max_record, limits,
                               prop_cases, run_props, walk_props, whole_command_at)


def run_golden(name):
    sc = SCENARIOS[name]
    g = golden_plane(dict(CFG, **sc.cfg))
    run = sc.fn(g, limits())
    return g, run, run_consumer(g, run.steps)


@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_golden_passes_the_model_free_checks(name):
    g, run, outs = run_golden(name)
    check_run(run, outs)
    if name.startswith("acks"):
        assert g.memory_in_use() == 0
        assert all(g.message_count(q.slot) == 0 for q in g.queues.values())
    if name == "frame_max":
        assert outs[0]["segs"] == [frame_max_record(run)]
    if name == "carry_too_large":
        assert (1, SS_TOO_LARGE, 0, 0) in outs[0]["segs"]


def test_golden_property_decode():
    """The model's reading of a publish's properties against the test's own byte-by-byte
    walk: persistence, expiry and timestamp of every case of ``prop_cases``."""
    from chanamq_amd.engine.golden import GoldenDataPlane
    g = GoldenDataPlane(persist=True, **{k: CFG[k] for k in GOLDEN_KEYS})
    cases, records, outs = run_props(g, NOW)
    check_props(g, cases, records, outs, NOW)


def test_property_walk_reads_the_cases_as_meant():
    """The walk itself, on values known by construction."""
    got = {name: walk_props(raw) for name, _, raw in prop_cases()}
    exp = [got[f"expiration {e!r}"] for e in EXPIRATIONS]
    assert exp == [(True, v, None) for v in (None, 0, 12, None, None, None, 12, None, None)]
    for n in range(18, 35):
        assert got[f"content_type {n}"] == (True, 40000 + n, 1_700_000_000 + n)
    assert got["all 14 properties"] == (True, 123456, 1_700_000_099)
    assert got["continuation word"] == (True, 40000, None)
    assert got["truncated list"] == got["truncated continuation"] == (False, None, None)


def test_limits_come_from_the_build():
    lim = limits()
    assert lim.FS_CAND_STAGED < lim.CAND_MAX and lim.FS_RUNS * 2 < lim.FS_CAND_STAGED
    assert lim.FS_STAGE % 16 == 0 and lim.FS_STAGE - 32 < lim.FS_AM_MAX * 16


def test_the_checks_bite():
    """The checks fail on the faults they are there for: a lost delivery, a doubled one, a
    segment record that loses bytes, a whole command left in a carry without SS_OVERFLOW, an
    error status on a well-formed stream, a carry left at the end."""
    from ingress_scenarios import check_deliveries, check_segments, pub
    g, run, outs = run_golden("look_failures")
    cut = [dict(o, egress={}) for o in outs]
    with pytest.raises(AssertionError):
        check_deliveries(cut, run.expect)
    twice = [dict(o, egress={c: e + e for c, e in o["egress"].items()}) for o in outs]
    with pytest.raises(AssertionError):
        check_deliveries(twice, run.expect)
    a, b = pub("x", b"one"), pub("x", b"two")
    assert whole_command_at(a) and not whole_command_at(a[:-1]) and len(list(commands(a + b + a[:9]))) == 2
    steps = [{1: a + b}, {}]
    ok = [dict(segs=[(1, 0, len(a + b), 0)]), dict(segs=[])]
    check_segments(steps, ok)
    lost = [dict(segs=[(1, 0, len(a), 0)]), dict(segs=[])]
    with pytest.raises(AssertionError, match="carry before"):
        check_segments(steps, lost)
    stalled = [dict(segs=[(1, 0, len(a), len(b))]), dict(segs=[(1, 0, len(b), 0)])]
    with pytest.raises(AssertionError, match="without SS_OVERFLOW"):
        check_segments(steps, stalled)
    kicked = [dict(segs=[(1, 32, len(a), len(b))]), dict(segs=[(1, 0, len(b), 0)])]
    check_segments(steps, kicked)
    with pytest.raises(AssertionError, match="well-formed"):
        check_segments(steps, [dict(segs=[(1, 4, len(a + b), 0)]), dict(segs=[])])
    with pytest.raises(AssertionError, match="carries left"):
        check_segments(steps[:1], kicked[:1])
