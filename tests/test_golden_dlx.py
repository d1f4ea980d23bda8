"""Dead-lettering on the golden model (CPU): every scenario of tests/dlx_scenarios.py, judged by the
scenarios' own record (``dlx_scenarios.check``: plain Python lists and the rules as CHANGES.md states
them, never the model).  This holds the golden model to the rules and shows that the inputs are
sound; tests/test_gpu_dlx.py holds the HIP data plane to the same record and to byte equality with
this model.  Plus ``ControlState``'s declare rule and the slot re-resolution."""

import pytest

from dlx_scenarios import OFF, SCENARIOS, cfg_of, check, golden_plane, run_dlx
from gpu_cfg import CFG

VH = "AMQ.DEFAULT"


@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_golden_keeps_the_rules(name):
    sc = SCENARIOS[name]
    g = golden_plane(cfg_of(sc, CFG))
    rec = sc.fn(g)
    check(rec, run_dlx(g, rec))
    if sc.drained:
        assert g.memory_in_use() == 0 and all(g.message_count(q.slot) == 0 for q in g.queues.values())
        assert not g.dead


@pytest.mark.parametrize("name", ["ttl_edges", "rejects", "routing"])
def test_off_ignores_the_arguments(name):
    """The scenarios with the option off are today's behaviour: nothing is dead-lettered."""
    sc = SCENARIOS[name]
    g = golden_plane(cfg_of(sc, CFG), on=False)
    rec = sc.fn(g, False)
    check(rec, run_dlx(g, rec))
    assert all(q.dlx is None for q in g.queues.values())


def test_off_is_today():
    g = golden_plane(dict(CFG), on=False)
    rec = OFF.fn(g)
    check(rec, run_dlx(g, rec))


def test_sharded_plane_is_refused():
    from chanamq_amd.engine.golden import GoldenDataPlane
    with pytest.raises(ValueError, match="sharded"):
        GoldenDataPlane(dead_letter=True, world=2, rank=0)


def test_declare_rule():
    """The key without the exchange, a value that is no string, a string above 255 bytes and a
    non-passive redeclare with another pair are 406 with nothing changed; a queue without a pair
    adopts the first non-passive declare's; the exchange need not exist, and its slot is looked up
    again at every exchange declare / delete that names it; off, the arguments are ignored."""
    from chanamq_amd.engine.control import ControlError, ControlState
    seen = []

    class C(ControlState):
        def queue_dlx_changed(self, q):
            seen.append((q.name, self.dlx_slot(q)))
    c = C(dead_letter=True)
    s = c.declare_queue(VH, "q", dead_letter_exchange="later", dead_letter_routing_key="k")
    q = c.queue_by_slot[s]
    assert (q.dlx, q.dlk) == ("later", b"k") and c.dlx_slot(q) is None
    assert c.declare_queue(VH, "q", dead_letter_exchange="later", dead_letter_routing_key="k") == s
    assert c.declare_queue(VH, "q") == s and c.declare_queue(VH, "q", passive=True, dead_letter_exchange="x") == s
    for kw in (dict(dead_letter_exchange="other", dead_letter_routing_key="k"), dict(dead_letter_exchange="later"),
               dict(dead_letter_exchange="later", dead_letter_routing_key="k2")):
        with pytest.raises(ControlError) as e:
            c.declare_queue(VH, "q", **kw)
        assert e.value.code == 406 and (q.dlx, q.dlk) == ("later", b"k")
    for kw in (dict(dead_letter_routing_key="k"), dict(dead_letter_exchange=5), dict(dead_letter_exchange="x" * 256),
               dict(dead_letter_exchange="x", dead_letter_routing_key=1.5),
               dict(dead_letter_exchange="x", dead_letter_routing_key="k" * 256)):
        with pytest.raises(ControlError) as e:
            c.declare_queue(VH, "new", **kw)
        assert e.value.code == 406 and (VH, "new") not in c.queues
    assert c.queue_by_slot[c.declare_queue(VH, "max", dead_letter_exchange="x" * 255)].dlx == "x" * 255
    # the exchange appears and goes: the slot is looked up again each time
    del seen[:]
    xs = c.declare_exchange(VH, "later", "fanout")
    assert seen == [("q", xs)] and c.dlx_slot(q) == xs
    c.delete_exchange(VH, "later")
    assert seen[-1] == ("q", None) and c.dlx_slot(q) is None
    # a queue without a pair (a recovered durable one) adopts the first non-passive declare's
    s2 = c.declare_queue(VH, "rec", durable=True)
    assert c.declare_queue(VH, "rec", durable=True, dead_letter_exchange="dx") == s2
    assert c.queue_by_slot[s2].dlx == "dx" and seen[-1] == ("rec", None)
    off = ControlState()
    assert off.queue_by_slot[off.declare_queue(VH, "q", dead_letter_exchange="x", dead_letter_routing_key=3)].dlx is None
