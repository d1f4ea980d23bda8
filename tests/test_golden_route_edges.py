"""The route / store / sort / enqueue scenarios of tests/route_scenarios.py on the golden model
(CPU), judged by ``route_scenarios.check_run``: what every consumer and every publisher must
see, worked out from the topology by the scenario's own brute-force matcher.  This holds the
model to the checks, proves every placement assertion of the scenarios (they run while a
scenario is built) and shows that the inputs are sound.  The model has no pair table, message
table or body log to fill: it runs the capacity scenarios with every publish expected whole.
tests/test_gpu_route_edges.py holds the HIP data plane to the same checks, with the limits,
and to byte equality with this model where a scenario is exact."""

import pytest

from gpu_cfg import CFG
from route_scenarios import (KEY_WIDTHS, SCENARIOS, SHARED, SORTING, TOPIC_PATTERNS, TOPIC_VECTORS, World, bits_for,
                             check_drained, check_run, golden_plane, limits, observe, run_route, sort_passes, sort_slots,
                             topic_hit, vector_queues, words)


def run_golden(sc, **over):
    g = golden_plane(dict(CFG, **sc.cfg, **over))
    run = sc.fn(g, limits())
    return g, run, run_route(g, run.steps, sc.now_step_ms)


@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_golden_passes_the_checks(name):
    sc = SCENARIOS[name]
    g, run, outs = run_golden(sc)
    check_run(run, outs, only=SHARED)
    if sc.drained:
        assert g.memory_in_use() == 0 and all(g.message_count(q.slot) == 0 for q in g.queues.values())


# (the model's run of sort_tiles differs between the widths only in the slots: the narrowest
# and the widest here, every width on the GPU)
SORT_CASES = [(name, q) for name in sorted(SORTING) for q in KEY_WIDTHS
              if name != "sort_tiles" or q in (KEY_WIDTHS[0], KEY_WIDTHS[-1])]


@pytest.mark.parametrize("name,q_max", SORT_CASES)
def test_golden_passes_the_sort_checks(name, q_max):
    sc = SORTING[name]
    g, run, outs = run_golden(sc, q_max=q_max)
    check_run(run, outs, only=SHARED)
    assert g.memory_in_use() == 0 and all(g.message_count(q.slot) == 0 for q in g.queues.values())
    slots = run.placed["slots"]
    assert slots[0] == 0 and slots[-1] == q_max - 1 and len(set(slots)) == len(slots)
    if q_max > 257:
        assert {255, 256} <= set(slots) and (len(slots) < 8 or 257 in slots)
    # every pass of the sort sees more than one digit (at q_max 1 << 16 the key has 17 bits and
    # no slot has the 17th: the third pass sorts one digit, and must still keep the order)
    digit, passes = sort_passes(q_max, limits())
    for p in range(passes):
        if (q_max - 1) >> (digit * p) == 0:
            continue
        assert len({(s >> (digit * p)) & ((1 << digit) - 1) for s in slots}) > 1, f"pass {p}"


def test_brute_force_matcher_agrees_with_the_reference_vectors():
    for key, want in TOPIC_VECTORS.items():
        assert vector_queues(key) == want.split(), key
    # the golden side's matcher on the same vectors (it is what the GPU is compared with)
    from chanamq_amd.models.matcher import topic_match
    for key, want in TOPIC_VECTORS.items():
        got = sorted(q for q, ps in TOPIC_PATTERNS.items() if any(topic_match(p, key) for p in ps))
        assert got == want.split(), key
    # '#' as a literal word (the reference's own reading)
    assert topic_hit(b"quote.#", b"quote.#", False) and not topic_hit(b"quote.#", b"quote.a", False)
    assert words(b"a..b.") == [b"a", b"", b"b"] and words(b"") == [b""] and words(b"...") == []


def test_limits_come_from_the_build():
    """A scenario aims at these: a constant that moves takes the scenario with it, and one
    that leaves the build fails here."""
    lim = limits()
    assert lim.SORT_TILE % 256 == 0 and lim.RS_RT >= 2 and lim.RS_RB >= 1
    assert 1 <= lim.PUB_QC < 64 and 8 < lim.SORT_ONEPASS_BITS < 16 and lim.TOPIC_WORDS == 8
    got = [sort_passes(q, lim) for q in KEY_WIDTHS]
    assert got == [(8, 1), (9, 1), (10, 1), (11, 1), (8, 2), (8, 3)], got
    assert bits_for(KEY_WIDTHS[3]) == lim.SORT_ONEPASS_BITS and bits_for(KEY_WIDTHS[4]) == lim.SORT_ONEPASS_BITS + 1
    assert sort_slots(1 << 16)[:2] == [0, 1] and len(sort_slots(128)) == 64


def test_the_checks_bite():
    """Each check fails on the fault it is there for: a lost delivery, a doubled one, two
    deliveries of one queue swapped, a Nack turned into an Ack (and the reverse), a lost
    return, a frame above the connection's frame-max, a counter off by one, a message that
    stays live."""
    from route_scenarios import ROUTING, check_confirms, check_counters, check_deliveries, check_returns
    g, run, outs = run_golden(SORTING["grow_many"], q_max=256)
    seen = observe(outs)
    check_deliveries(run, seen)
    dl = [i for i, s in enumerate(seen) if s.kind == "deliver" and s.ctag == "g4"]
    with pytest.raises(AssertionError, match="lost publishes"):
        check_deliveries(run, retag(seen[:dl[3]] + seen[dl[3] + 1:]))
    with pytest.raises(AssertionError, match="delivered twice"):
        check_deliveries(run, retag(seen[:dl[3]] + [seen[dl[3]]] + seen[dl[3]:]))
    swapped = list(seen)
    swapped[dl[3]], swapped[dl[4]] = seen[dl[4]]._replace(tag=seen[dl[3]].tag), seen[dl[3]]._replace(tag=seen[dl[4]].tag)
    with pytest.raises(AssertionError, match="out of publish order"):
        check_deliveries(run, swapped)
    other = [i for i, s in enumerate(seen) if s.kind == "deliver" and s.ctag == "g3"][0]
    with pytest.raises(AssertionError, match="not routed to it"):
        check_deliveries(run, retag(seen[:dl[3]] + [seen[dl[3]]._replace(body=seen[other].body)] + seen[dl[3]:]))
    check_confirms(run, seen)
    nacks = [i for i, s in enumerate(seen) if s.kind == "nack"]
    assert len(nacks) == 1
    with pytest.raises(AssertionError, match="confirm"):
        check_confirms(run, [s._replace(kind="ack") if i == nacks[0] else s for i, s in enumerate(seen)])
    acks = [i for i, s in enumerate(seen) if s.kind == "ack"]
    with pytest.raises(AssertionError, match="confirm"):
        check_confirms(run, [s._replace(kind="nack") if i == acks[0] else s for i, s in enumerate(seen)])
    with pytest.raises(AssertionError, match="confirms, expected"):
        check_confirms(run, [s for i, s in enumerate(seen) if i != acks[-1]])
    check_counters(run, outs, only=SHARED)
    off = [dict(o, counters=dict(o["counters"], n_ring_full=o["counters"].get("n_ring_full", 0) + 1)) for o in outs]
    with pytest.raises(AssertionError, match="n_ring_full"):
        check_counters(run, off, only=SHARED)
    g, run, outs = run_golden(ROUTING["mixed_group"])
    seen = observe(outs)
    check_returns(run, seen)
    rets = [i for i, s in enumerate(seen) if s.kind == "return"]
    with pytest.raises(AssertionError, match="returns"):
        check_returns(run, [s for i, s in enumerate(seen) if i != rets[2]])
    swapped = list(seen)
    swapped[rets[0]], swapped[rets[1]] = seen[rets[1]], seen[rets[0]]
    with pytest.raises(AssertionError, match="publish order"):
        check_returns(run, swapped)
    from route_scenarios import MIXED_FM, check_frames
    check_frames(run, seen)
    long = [i for i, s in enumerate(seen) if s.kind == "return" and len(s.body) > MIXED_FM]
    assert long and all(seen[i].frame == MIXED_FM for i in long)      # split at the publisher's frame-max
    with pytest.raises(AssertionError, match="frame-max"):
        check_frames(run, [s._replace(frame=MIXED_FM + 1) if i == long[0] else s for i, s in enumerate(seen)])
    check_drained(dict(n_live_msgs=0, live_bytes=0, log_head=5000, log_tail=4096), 4096)
    with pytest.raises(AssertionError, match="still live"):
        check_drained(dict(n_live_msgs=1, live_bytes=0, log_head=0, log_tail=0), 4096)
    with pytest.raises(AssertionError, match="log bytes still live"):
        check_drained(dict(n_live_msgs=0, live_bytes=1024, log_head=0, log_tail=0), 4096)
    with pytest.raises(AssertionError, match="behind the head"):
        check_drained(dict(n_live_msgs=0, live_bytes=0, log_head=3 * 4096, log_tail=4096), 4096)


def retag(seen):
    """Delivery tags counted again (a lost or doubled delivery is judged by its queue, not by
    the hole it leaves in the channel's tags)."""
    nxt, out = {}, []
    for s in seen:
        if s.kind == "deliver":
            nxt[(s.conn, s.ch)] = nxt.get((s.conn, s.ch), 0) + 1
            s = s._replace(tag=nxt[(s.conn, s.ch)])
        out.append(s)
    return out


def test_world_routes_by_its_own_record():
    """The expectation side on a topology small enough to read: direct by key, fanout to all,
    topic by words, the default exchange by queue name, an unknown exchange to nobody."""
    g = golden_plane(CFG)
    w = World(g)
    w.exchange("d", "direct")
    w.exchange("f", "fanout")
    w.exchange("t", "topic")
    for q in ("a", "b", "c"):
        w.queue(q)
    w.bind("b", "d", "k")
    w.bind("a", "d", "k")
    w.bind("c", "f", "")
    w.bind("a", "f", "x")
    w.bind("b", "t", "x.*")
    w.bind("c", "t", "#.y")
    assert w.route("d", "k") == ["a", "b"] and w.route("d", "j") == [] and w.route("f", "zz") == ["a", "c"]
    assert w.route("t", "x.y") == ["b", "c"] and w.route("t", "y") == ["c"] and w.route("t", "x") == []
    assert w.route("", "b") == ["b"] and w.route("", "k") == [] and w.route("nope", "k") is None
