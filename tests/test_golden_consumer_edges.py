"""The consumer-half scenarios on the golden model (CPU): each test states what the clients
must observe, decoded from the egress and judged by ``consumer_scenarios.CHECKS`` -- from the
protocol, never from the model.  tests/test_gpu_consumer_edges.py holds the HIP data plane
to the same statements and to byte equality with this model."""

import pytest

from consumer_scenarios import CHECKS, FOLDED, SCENARIOS, ck_folded_settles_mixed, golden_plane, run_consumer
from gpu_cfg import CFG


def run_golden(sc):
    g = golden_plane(dict(CFG, **sc.cfg))
    return g, run_consumer(g, sc.fn(g), sc.now_step_ms)


def check(name):
    g, outs = run_golden(SCENARIOS[name])
    CHECKS[name](outs)
    return g, outs


def test_window_chunks():
    """Tags 1..600 in order; the one nack-requeued body (tag 400) comes back flagged as tag
    601; with prefetch 0 a burst delivers exactly the window's free slots, so every step's
    count says where the head is: 1747 after the multiple ack of 300, then 64, 191, and after
    the ack of everything 46 and 2002."""
    check("window_chunks")


def test_many_settles():
    """256 alternating multiple settles: exactly tags 3-4, 7-8, .., 511-512 come back, in
    queue order, flagged.  300 multiple acks: all 300 credits return (the second 300 arrive in
    the same step).  256 acks and a nack-requeue of 300: exactly 257..300 come back."""
    g, _ = check("many_settles")
    assert g.memory_in_use() == 0


def test_folded_settles_mixed_invariants_hold_for_exact_resolution_too():
    """The invariants asked of the engine's fold past MS_MAX also hold for the model's
    exact resolution (259-260 back, 257-258 acked)."""
    _, outs = run_golden(FOLDED)
    ck_folded_settles_mixed(outs)


@pytest.mark.parametrize("name", ["requeue_1024", "requeue_1025", "requeue_two_queues"])
def test_requeue_keeps_queue_order(name):
    """basic.nack(0, multiple, requeue) of 1024 / 1025 / 513 + 512 deliveries: the same bodies
    again in the same step, per queue in their first order, all flagged, tags counting on."""
    g, _ = check(name)
    assert g.memory_in_use() == 0


def test_requeue_partial():
    """1100 requeued into a ring with 1048 free slots: the 1048 lowest come back at once, in
    order and flagged, ahead of the 1000 that were waiting; the other 52 once there is room."""
    g, _ = check("requeue_partial")
    assert g.memory_in_use() == 0


def test_requeue_full_ring():
    """8 requeued into a ring with 3 free slots: 3 come back at once (lowest first), 5 when
    there is room; 21 bodies, each delivered once plus the 8 once more with the flag; never
    more than prefetch 8 unacked."""
    g, _ = check("requeue_full_ring")
    assert g.memory_in_use() == 0


def test_global_prefetch():
    """The channel with qos(5, global) never holds more than 5 unacked over its two
    consumers; the per-consumer channel holds up to 5 for each; 12 messages of each queue are
    delivered exactly once."""
    check("global_prefetch")


def test_flow_and_cancel():
    """Each step hands out the head of the queue, split in ceil shares from the round-robin
    start; a channel with flow off, a cancelled consumer and one not yet attached get
    nothing; every message exactly once."""
    check("flow_and_cancel")


def test_seventy_consumers():
    """64 of 70 consumers are served a step, from a start that moves on by one; each run is
    the next stretch of the queue; with 3 messages the first 3 in the walk get one each."""
    check("seventy_consumers")


def test_gets_squeeze_consumers():
    """32 GetOk (tags 1..32, message-count 99 down to 68), the 33rd Get handed to the host,
    the other 68 messages split over the first 32 consumers of the walk."""
    check("gets_squeeze_consumers")


def test_ttl_waves():
    """Backlogs of 64, 65 and 130 expire in the step the fresh message arrives behind them,
    which survives; it expires alone two steps later; the consumer gets only the last one."""
    g, _ = check("ttl_waves")
    assert g.memory_in_use() == 0


def test_consumer_frame_max():
    """frame-max 4096: body frames of at most 4088 bytes -- none for an empty body, 4088 +
    4088 + 1 for 8177 -- for Basic.Deliver and GetOk alike."""
    check("consumer_frame_max")


def test_deliver_cap_multi():
    """deliver_cap 64 and three consumers on 500: 64 each for two steps, then 39, 39, 38."""
    check("deliver_cap_multi")


def test_every_scenario_has_a_check():
    assert sorted(CHECKS) == sorted(SCENARIOS)
