"""Priority queues in the golden model: every scenario of tests/prio_scenarios.py judged by the
scenarios' own record (a list of FIFOs per priority, written without the model), at both q_max
widths; the control plane's rules for x-max-priority (lanes, slots, 406 and 506)."""

import pytest

from chanamq_amd.engine.control import ControlError, ControlState
from chanamq_amd.engine.golden import GoldenDataPlane
from dp_scenarios import VH
from gpu_cfg import CFG
from prio_scenarios import OFF, SCENARIOS, WIDTHS, cfg_of, check, golden_plane, run_prio


@pytest.mark.parametrize("width", sorted(WIDTHS))
@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_prio(name, width):
    sc = SCENARIOS[name]
    g = golden_plane(dict(cfg_of(sc, CFG), **WIDTHS[width]))
    rec = sc.fn(g)
    check(rec, run_prio(g, rec))
    if sc.drained:
        assert all(g.message_count(q.slot) == 0 for q in g.queues.values())


def test_off_is_today():
    g = golden_plane(CFG, on=False)
    rec = OFF.fn(g, False)
    check(rec, run_prio(g, rec))
    assert len(g.queue_by_slot) == 1 and g.queues[(VH, "of")].max_priority is None


def code(fn, *a, **kw):
    with pytest.raises(ControlError) as e:
        fn(*a, **kw)
    return e.value.code, e.value.text


def test_declare_rules():
    cs = ControlState(q_max=16, priority_queues=True, queue_limits=True, queue_limit_bytes=True)
    for bad in (0, 16, 255, -1, True, "3", 2.0, None):
        if bad is None:
            continue
        c, text = code(cs.declare_queue, VH, "bad", max_priority=bad)
        assert c == 406 and "15" in text
    assert not cs.queues and len(cs._free_q) == 16
    s = cs.declare_queue(VH, "p", max_priority=3)
    q = cs.queues[(VH, "p")]
    assert [lq.slot for lq in q.lanes] == [s, s + 1, s + 2, s + 3] and q.max_priority == 3
    assert all(cs.queue_by_slot[s + k].lane_of == s for k in (1, 2, 3)) and q.lane_of == -1
    assert [x for x in cs.queues.values()] == [q]
    assert [b for b in cs.exchanges[(VH, "")].bindings] == [(s, b"p")]
    assert cs.declare_queue(VH, "p") == s                       # no argument: the queue as it is
    assert cs.declare_queue(VH, "p", max_priority=3) == s
    assert code(cs.declare_queue, VH, "p", max_priority=4)[0] == 406
    plain = cs.declare_queue(VH, "plain")
    c, text = code(cs.declare_queue, VH, "plain", max_priority=2)   # nothing is adopted later
    assert c == 406 and "without" in text
    assert code(cs.declare_queue, VH, "l", max_priority=2, max_length=5)[0] == 406
    assert code(cs.declare_queue, VH, "l", max_priority=2, max_length_bytes=5)[0] == 406
    assert code(cs.declare_queue, VH, "p", max_length=5)[0] == 406
    assert (VH, "l") not in cs.queues and plain == s + 4


def test_slots_come_back_and_need_a_run():
    cs = ControlState(q_max=8, priority_queues=True)
    a = cs.declare_queue(VH, "a", max_priority=2)      # 0..2
    b = cs.declare_queue(VH, "b")                      # 3
    c = cs.declare_queue(VH, "c", max_priority=3)      # 4..7
    assert (a, b, c) == (0, 3, 4)
    assert code(cs.declare_queue, VH, "full")[0] == 506
    cs.delete_queue(VH, "b")
    c506, text = code(cs.declare_queue, VH, "d", max_priority=1)   # one slot free: no run of two
    assert c506 == 506 and "consecutive" in text
    assert cs.declare_queue(VH, "b2") == 3
    cs.delete_queue(VH, "a")
    assert sorted(cs._free_q) == [0, 1, 2] and set(cs.queue_by_slot) == {3, 4, 5, 6, 7}
    assert cs.declare_queue(VH, "d", max_priority=1) in (0, 1)
    assert code(cs.declare_queue, VH, "e", max_priority=1)[0] == 506   # one slot is left
    cs.delete_queue(VH, "c")
    assert cs.declare_queue(VH, "e", max_priority=3) == 4


def test_durable_with_store_and_sharding_are_refused():
    g = GoldenDataPlane(persist=True, priority_queues=True)
    assert code(g.declare_queue, VH, "d", durable=True, max_priority=2)[0] == 406
    assert g.declare_queue(VH, "t", max_priority=2) == 0            # transient: served
    with pytest.raises(ValueError):
        ControlState(world=2, priority_queues=True)


def test_exclusive_owner_cleanup_and_counts():
    g = GoldenDataPlane(priority_queues=True, q_max=16)
    g.open_connection(1, VH)
    s = g.declare_queue(VH, "x", exclusive_owner=1, max_priority=2)
    assert g.lane_slots(s) == [s, s + 1, s + 2]
    g.close_connection(1)
    assert not g.queues and not g.queue_by_slot and len(g._free_q) == 16
