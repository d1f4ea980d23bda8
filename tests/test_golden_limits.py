"""Queue length limits on the golden model (CPU): every scenario of tests/limit_scenarios.py,
judged by the scenarios' own record (``limit_scenarios.check``: a Python list per queue and the
rules as they are written down, never the model).  This holds the golden model to the rules
and shows that the inputs are sound; tests/test_gpu_limits.py holds the HIP data plane to the
same record and to byte equality with this model.  Plus ``ControlState``'s declare rule."""

import pytest

from gpu_cfg import CFG
from limit_scenarios import OFF, SCENARIOS, cfg_of, check, golden_plane, run_limits, sharded_check, sharded_cluster, sharded_run

VH = "AMQ.DEFAULT"


@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_golden_keeps_the_rules(name):
    sc = SCENARIOS[name]
    g = golden_plane(cfg_of(sc, CFG))
    rec = sc.fn(g)
    check(rec, run_limits(g, rec))
    if sc.drained:
        assert g.memory_in_use() == 0 and all(g.message_count(q.slot) == 0 for q in g.queues.values())


def test_off_is_today():
    """The option off: the arguments are ignored, neither counter moves."""
    g = golden_plane(dict(CFG), on=False)
    rec = OFF.fn(g)
    check(rec, run_limits(g, rec))


@pytest.mark.parametrize("lag", [0, 1])
def test_golden_cluster_owner_enforces(lag):
    sharded_check(sharded_run(sharded_cluster(CFG, lag)))


def test_declare_rule():
    """A declare of an existing queue returns its slot; a limit or mode that differs is 406; a
    queue without a limit adopts the first non-passive declare's; invalid values are 406 with
    nothing changed; with the option off the arguments are ignored."""
    from chanamq_amd.engine.control import ControlError, ControlState
    c = ControlState(queue_limits=True)
    s = c.declare_queue(VH, "q", max_length=5)
    q = c.queue_by_slot[s]
    assert (q.max_length, q.overflow) == (5, "drop-head")
    assert c.declare_queue(VH, "q", max_length=5, overflow="drop-head") == s
    assert c.declare_queue(VH, "q") == s and c.declare_queue(VH, "q", passive=True, max_length=9) == s
    for kw in (dict(max_length=6), dict(max_length=5, overflow="reject-publish")):
        with pytest.raises(ControlError) as e:
            c.declare_queue(VH, "q", **kw)
        assert e.value.code == 406 and (q.max_length, q.overflow) == (5, "drop-head")
    for kw in (dict(max_length=-1), dict(max_length="5"), dict(max_length=2.0), dict(max_length=True),
               dict(max_length=1, overflow="reject-publish-dlx"), dict(max_length=1, overflow=3)):
        with pytest.raises(ControlError) as e:
            c.declare_queue(VH, "new", **kw)
        assert e.value.code == 406 and (VH, "new") not in c.queues
    s0 = c.declare_queue(VH, "zero", max_length=0, overflow="reject-publish")
    assert (c.queue_by_slot[s0].max_length, c.queue_by_slot[s0].overflow) == (0, "reject-publish")
    # a queue without a limit (a recovered one): a passive declare changes nothing, the first
    # non-passive declare with a limit is adopted, the next one must agree
    r = c.declare_queue(VH, "rec", durable=True)
    c.declare_queue(VH, "rec", passive=True, max_length=3)
    assert c.queue_by_slot[r].max_length is None
    assert c.declare_queue(VH, "rec", durable=True, max_length=3, overflow="reject-publish") == r
    assert (c.queue_by_slot[r].max_length, c.queue_by_slot[r].overflow) == (3, "reject-publish")
    with pytest.raises(ControlError) as e:
        c.declare_queue(VH, "rec", max_length=4, overflow="reject-publish")
    assert e.value.code == 406
    off = ControlState()
    so = off.declare_queue(VH, "q", max_length=-7, overflow="whatever")
    assert off.queue_by_slot[so].max_length is None and off.declare_queue(VH, "q", max_length=1) == so


def test_control_log_carries_the_limit():
    """Every replica applies the same rule: the limit travels in the op's keywords."""
    from chanamq_amd.engine.control import ControlState
    from chanamq_amd.parallel.control_log import ControlLog
    import json
    a, b = ControlState(queue_limits=True), ControlState(queue_limits=True)
    log = ControlLog(a, None)
    log.submit("declare_queue", VH, "lq", durable=True, max_length=7, overflow="reject-publish")
    op, args, kw = json.loads(json.dumps(log.outbox[0]))
    for p in (a, b):
        getattr(p, op)(*args, **kw)
        q = p.queues[(VH, "lq")]
        assert (q.max_length, q.overflow, q.durable) == (7, "reject-publish", True)
