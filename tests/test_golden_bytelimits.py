"""Queue byte limits on the golden model (CPU): every scenario of tests/bytelimit_scenarios.py,
judged by the scenarios' own record (``bytelimit_scenarios.check``: a Python list per queue and
the rule as it is written down, never the model), at both pair-key widths.  This holds the golden
model to the rule and shows that the inputs are sound; tests/test_gpu_bytelimits.py holds the HIP
data plane to the same record and to equality with this model.  Plus ``ControlState``'s declare
rule, the control log's keywords and the reload that lifts the limit."""

import pytest

from bytelimit_scenarios import (OFF, SCENARIOS, WIDTHS, cfg_of, check, golden_plane, run_bytes, sharded_check,
                                 sharded_cluster, sharded_run, x_death_reasons)
from gpu_cfg import CFG

VH = "AMQ.DEFAULT"


@pytest.mark.parametrize("width", sorted(WIDTHS))
@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_golden_keeps_the_rule(name, width):
    sc = SCENARIOS[name]
    g = golden_plane(dict(cfg_of(sc, CFG), **WIDTHS[width]))
    rec = sc.fn(g)
    outs = run_bytes(g, rec)
    check(rec, outs)
    if sc.drained:
        assert g.memory_in_use() == 0 and all(g.message_count(q.slot) == 0 for q in g.queues.values())
    if sc.cfg.get("x_death"):
        assert x_death_reasons(outs, 2, 1) == ["maxlen"] * len(rec.died)


def test_off_is_today():
    """``queue_limits`` on, the byte flag off: the keyword is ignored."""
    g = golden_plane(dict(CFG), on=False)
    assert not g.queue_limit_bytes
    rec = OFF.fn(g)
    check(rec, run_bytes(g, rec))
    assert all(q.max_length_bytes is None for q in g.queues.values())


@pytest.mark.parametrize("lag", [0, 1])
def test_golden_cluster_owner_enforces(lag):
    sharded_check(sharded_run(sharded_cluster(CFG, lag)))


def test_flag_needs_queue_limits():
    from chanamq_amd.engine.control import ControlState
    from chanamq_amd.engine.golden import GoldenDataPlane
    for cls in (ControlState, GoldenDataPlane):
        with pytest.raises(ValueError):
            cls(queue_limit_bytes=True)
        assert cls(queue_limits=True, queue_limit_bytes=True).queue_limit_bytes


def test_declare_rule():
    """A value that differs from the queue's is 406, and so is a mode that differs; a queue
    without a byte limit adopts the first non-passive declare's; a redeclare without the
    argument is a no-op; invalid values are 406 with nothing changed; the value is kept in 64
    bits; either limit may be set without the other."""
    from chanamq_amd.engine.control import ControlError, ControlState
    c = ControlState(queue_limits=True, queue_limit_bytes=True)
    s = c.declare_queue(VH, "q", max_length_bytes=(1 << 32) + 5)
    q = c.queue_by_slot[s]
    assert (q.max_length, q.max_length_bytes, q.overflow) == (None, (1 << 32) + 5, "drop-head")
    assert c.declare_queue(VH, "q", max_length_bytes=(1 << 32) + 5, overflow="drop-head") == s
    assert c.declare_queue(VH, "q") == s and c.declare_queue(VH, "q", passive=True, max_length_bytes=9) == s
    for kw in (dict(max_length_bytes=5), dict(max_length_bytes=(1 << 32) + 5, overflow="reject-publish"),
               dict(max_length=3, overflow="reject-publish")):
        with pytest.raises(ControlError) as e:
            c.declare_queue(VH, "q", **kw)
        assert e.value.code == 406 and (q.max_length, q.max_length_bytes, q.overflow) == (None, (1 << 32) + 5, "drop-head")
    # the count limit joins a queue that has the byte limit alone, under the queue's mode
    assert c.declare_queue(VH, "q", max_length=3) == s and (q.max_length, q.max_length_bytes) == (3, (1 << 32) + 5)
    for kw in (dict(max_length_bytes=-1), dict(max_length_bytes="5"), dict(max_length_bytes=2.0), dict(max_length_bytes=True),
               dict(max_length_bytes=1, overflow="reject-publish-dlx"), dict(max_length=1, max_length_bytes=None, overflow=3)):
        with pytest.raises(ControlError) as e:
            c.declare_queue(VH, "new", **kw)
        assert e.value.code == 406 and (VH, "new") not in c.queues
    z = c.queue_by_slot[c.declare_queue(VH, "zero", max_length_bytes=0, overflow="reject-publish")]
    assert (z.max_length_bytes, z.overflow) == (0, "reject-publish")
    # a recovered queue (no limit stored): the first non-passive declare's value is adopted
    r = c.declare_queue(VH, "rec", durable=True, max_length=4, overflow="reject-publish")
    c.declare_queue(VH, "rec", passive=True, max_length_bytes=3)
    assert c.queue_by_slot[r].max_length_bytes is None
    assert c.declare_queue(VH, "rec", durable=True, max_length_bytes=3, overflow="reject-publish") == r
    assert (c.queue_by_slot[r].max_length, c.queue_by_slot[r].max_length_bytes) == (4, 3)
    with pytest.raises(ControlError) as e:
        c.declare_queue(VH, "rec", max_length_bytes=4, overflow="reject-publish")
    assert e.value.code == 406
    # the flag off: the keyword is ignored, whatever it holds
    off = ControlState(queue_limits=True)
    so = off.declare_queue(VH, "q", max_length_bytes=-7)
    assert off.queue_by_slot[so].max_length_bytes is None and off.declare_queue(VH, "q", max_length_bytes=1) == so


def test_control_log_carries_the_limit():
    """Every replica applies the same rule: the limit travels in the op's keywords."""
    import json

    from chanamq_amd.engine.control import ControlState
    from chanamq_amd.parallel.control_log import ControlLog
    kw = dict(queue_limits=True, queue_limit_bytes=True)
    a, b = ControlState(**kw), ControlState(**kw)
    log = ControlLog(a, None)
    log.submit("declare_queue", VH, "lq", durable=True, max_length_bytes=(1 << 40) + 1, overflow="reject-publish")
    op, args, kw = json.loads(json.dumps(log.outbox[0]))
    for p in (a, b):
        getattr(p, op)(*args, **kw)
        q = p.queues[(VH, "lq")]
        assert (q.max_length_bytes, q.overflow, q.durable) == ((1 << 40) + 1, "reject-publish", True)


def test_reload_lifts_the_limit_and_counts_the_bytes():
    """A reload is never refused: the limits are lifted while the messages are restored and put
    back afterwards, and the restored entries' bytes are counted."""
    from chanamq_amd.engine.persistence import GpuPersistence
    g = golden_plane(dict(CFG))
    slot = g.declare_queue(VH, "rq", durable=True, max_length_bytes=10, overflow="reject-publish")
    seen = []
    restore = g.restore
    g.restore = lambda items, now_ms=0: (seen.append(g.queue_by_slot[slot].max_length_bytes), restore(items, now_ms))[1]
    pers = GpuPersistence.__new__(GpuPersistence)
    pers.plane = g
    items = [(slot, 100 + i, 0, 0, b"", b"rq", b"", b"x" * 8, True, False) for i in range(3)]
    assert pers._reload(items, 0) == 3 and seen == [None]
    q = g.queue_by_slot[slot]
    assert (q.max_length_bytes, q.overflow) == (10, "reject-publish") and g.queue_bytes(slot) == 24
