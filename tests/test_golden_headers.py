"""The headers-exchange scenarios of tests/headers_scenarios.py on the golden model (CPU),
judged by ``route_scenarios.check_run`` from the scenarios' own brute-force matcher: this holds
``models/matcher.py`` and the golden model's routing to the rule, proves every placement
assertion of the scenarios and shows that the inputs are sound.  tests/test_gpu_headers.py
holds the HIP data plane to the same checks and to byte equality with this model."""

import pytest

from chanamq_amd.protocol.codec import Typed
from gpu_cfg import CFG
from headers_scenarios import (NAME_PAIR, OFF, SCENARIOS, VALUE_PAIR, brute_match, cfg_of, fnv32, golden_plane, limits,
                               props_bytes, table_body)
from route_scenarios import SHARED, check_run, run_route


@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_golden_passes_the_checks(name):
    sc, lim = SCENARIOS[name], limits()
    g = golden_plane(cfg_of(sc, CFG, lim))
    run = sc.fn(g, lim)
    outs = run_route(g, run.steps, sc.now_step_ms)
    check_run(run, outs, only=SHARED)
    if sc.drained:
        assert g.memory_in_use() == 0 and all(g.message_count(q.slot) == 0 for q in g.queues.values())


def test_off_is_today():
    """The option off: a headers exchange routes as topic and arguments are ignored."""
    g = golden_plane(dict(CFG), headers_match=False)
    run = OFF.fn(g, None)
    check_run(run, run_route(g, run.steps), only=SHARED)


def test_limits_come_from_the_build():
    lim = limits()
    assert 1 <= lim.HB_PAIRS <= 32 and 1 <= lim.PUB_QC < 64


def test_brute_force_matcher_by_hand():
    """The expectation side on vectors small enough to read, and the golden side's matcher
    (what the GPU is compared with) on the same."""
    from chanamq_amd.models.matcher import canon_args, fnv1a32, headers_match, props_headers
    vectors = [
        ({"x-match": "all", "a": "1", "b": "2"}, [("a", "1"), ("b", "2")], True),
        ({"x-match": "all", "a": "1", "b": "2"}, [("a", "1")], False),
        ({"x-match": "any", "a": "1", "b": "2"}, [("b", "2")], True),
        ({"x-match": "any", "a": "1", "b": "2"}, [("c", "2")], False),
        ({"x-match": "any"}, None, True), ({}, [], True), ({"x-y": "1"}, None, True),
        ({"x-match": "other", "a": "1"}, [("a", "2")], False),
        ({"a": None}, [("a", Typed("d", 2.5))], True), ({"a": None}, [("b", "1")], False),
        ({"a": "5"}, [("a", Typed("b", 5))], True), ({"a": "5"}, [("a", Typed("l", 5))], True),
        ({"a": Typed("u", 5)}, [("a", "5")], True), ({"a": "5"}, [("a", "6"), ("a", "5")], False),
        ({"a": "true"}, [("a", True)], True), ({"a": ""}, [("a", None)], True),
        ({"a": 2.5}, [("a", 2.5)], True), ({"a": 2.5}, [("a", Typed("f", 2.5))], False),
        ({"a": 2.5}, [("a", "2.5")], False), ({"a": "d"}, [("a", 2.5)], False),
        ({"a": "-9223372036854775808"}, [("a", Typed("T", 1 << 63))], True),
    ]
    for args, hdrs, want in vectors:
        assert brute_match(args, hdrs) is want, (args, hdrs)
        props = props_bytes(hdrs)
        assert headers_match(args, props) is want, (args, hdrs)
        assert headers_match(canon_args(args), props_headers(props)) is want
    for a, b in (NAME_PAIR, VALUE_PAIR):
        assert fnv1a32(a.encode()) == fnv1a32(b.encode()) == fnv32(a.encode())
    # a table cut inside an entry, an unknown tag: no headers at all, whatever came before
    good = table_body([("a", "1")])
    assert props_headers(props_bytes(table=(len(good) + 3).to_bytes(4, "big") + good + b"\x01bU")) == {}
    assert props_headers(props_bytes(table=(len(good) + 5).to_bytes(4, "big") + good)) == {}
    assert props_headers(b"") == {} and props_headers(props_bytes([("a", "1")])) == {b"a": (0, b"1")}


def test_bindings_are_kept_by_their_canonical_arguments():
    """Identity, duplicates, unbind, and the topic table left alone."""
    from chanamq_amd.engine.control import ControlState
    VH = "AMQ.DEFAULT"
    c = ControlState(headers_match=True)
    c.tb_max = 0          # not one topic row may be taken
    c.declare_exchange(VH, "h", "headers")
    c.declare_exchange(VH, "h2", "headers")
    c.declare_queue(VH, "q")
    x = c.exchanges[(VH, "h")]
    c.bind(VH, "q", "h", "k", {"a": 5, "x-match": "all"})
    c.bind(VH, "q", "h", "k", {"a": "5"})                 # the same canonical arguments: a no-op
    c.bind(VH, "q", "h", "k", {"a": Typed("l", 5), "x-other": 1})
    assert len(x.hbindings) == 1 and not x.bindings
    c.bind(VH, "q", "h", "k", {"a": "5", "x-match": "any"})
    c.bind(VH, "q", "h", "other", {"a": "5"})
    c.bind(VH, "q", "h", "k", {"a": None})
    assert len(x.hbindings) == 4
    c.bind_exchange(VH, "h2", "h", "", {"a": "5"})        # (tb_max 0: an edge takes no topic row either)
    c.bind_exchange(VH, "h2", "h", "", {"a": Typed("B", 5)})
    assert len(x.hxbindings) == 1
    c.unbind(VH, "q", "h", "k", {"a": "6"})
    assert len(x.hbindings) == 4
    c.unbind(VH, "q", "h", "k", {"a": Typed("s", 5)})
    assert len(x.hbindings) == 3 and all(b[2] != (False, ((b"a", False, 0, b"5"),)) or b[1] != b"k" for b in x.hbindings)
    c.unbind_exchange(VH, "h2", "h", "", {"a": "5"})
    assert not x.hxbindings
    c.delete_queue(VH, "q")
    assert not x.hbindings
    # off: arguments are ignored and the binding is a topic row
    c = ControlState()
    c.declare_exchange(VH, "h", "headers")
    c.declare_queue(VH, "q")
    c.bind(VH, "q", "h", "k", {"a": 5})
    c.bind(VH, "q", "h", "k", {"a": 6})
    assert c.exchanges[(VH, "h")].bindings == [(c.queues[(VH, "q")].slot, b"k")] and not c.exchanges[(VH, "h")].hbindings


@pytest.mark.parametrize("lag", [0, 1])
@pytest.mark.parametrize("world", [2, 3])
def test_golden_cluster_rematches_from_the_record(world, lag):
    """A headers publish whose queues live on other ranks: the owner matches again from the
    record's own property bytes."""
    from headers_scenarios import sharded_cluster, sharded_got, sharded_run
    outs, want = sharded_run(sharded_cluster(CFG, world, lag))
    assert sharded_got(outs) == {q: v for q, v in want.items() if v}


def test_host_routing_takes_the_property_bytes():
    """``ControlState.route_host`` (large publishes assembled on the host, the sharded blob
    path) with a publish's property bytes: a headers exchange, an edge out of it matched on
    arguments, and the walk beyond -- the same list, in the same order, as the golden model's
    own routing, and the sets the brute-force matcher names."""
    from chanamq_amd.engine.control import ControlState
    VH = "AMQ.DEFAULT"
    g = golden_plane(dict(CFG))
    c = ControlState(headers_match=True)
    binds = [("q1", "h", {"a": "1"}), ("q2", "h", {"x-match": "any", "a": "1", "b": Typed("I", 2)}), ("q3", "h", {})]
    edge = {"go": None}
    for p in (g, c):
        p.declare_exchange(VH, "h", "headers")
        p.declare_exchange(VH, "t", "topic")
        for q in ("q1", "q2", "q3", "far"):
            p.declare_queue(VH, q)
        for q, x, a in binds:
            p.bind(VH, q, x, "ignored", a)
        p.bind(VH, "far", "t", "k.*")
        p.bind_exchange(VH, "t", "h", "", edge)
    slot = {q.name: q.slot for q in c.queues.values()}
    for hdrs, key in (([("a", "1")], "k.1"), ([("b", "2"), ("go", 0)], "k.1"), ([("go", "x")], "other"), (None, "k.1"),
                      ([("a", Typed("B", 1)), ("a", "2"), ("go", "")], "k.9")):
        props = props_bytes(hdrs)
        want = {q for q, _, a in binds if brute_match(a, hdrs)} | (
            {"far"} if brute_match(edge, hdrs) and key.startswith("k.") else set())
        x = c.exchanges[(VH, "h")]
        got = c.route_host(x, key.encode(), props)
        assert {n for n, s in slot.items() if s in got} == want and len(got) == len(want), (hdrs, key)
        assert g._route(g.exchanges[(VH, "h")], key.encode(), props) == got
    assert c.route_host(c.exchanges[(VH, "h")], b"k.1") == [slot["q3"]]          # no property bytes: no headers


def test_key_pool_room_and_reach_are_refused_at_bind_time():
    """The fourth bound: the names and values of a headers binding need room in the key pool
    beside the other tables' keys and patterns.  And a headers exchange is routed as a walk,
    so it binds at most ``hop_qmax`` distinct queues.  506, nothing changed."""
    from chanamq_amd.engine.control import ControlError, ControlState
    VH = "AMQ.DEFAULT"
    c = ControlState(headers_match=True)
    c.declare_exchange(VH, "h", "headers")
    c.declare_exchange(VH, "t", "topic")
    c.declare_exchange(VH, "d", "direct")
    for q in ("q", "r", "s"):
        c.declare_queue(VH, q)
    base = c.kpool_bytes()
    c.bind(VH, "q", "t", "pattern.*")
    c.bind(VH, "q", "d", "key")
    c.bind(VH, "r", "d", "key")                       # a direct key is held once
    assert c.kpool_bytes() == base + len("pattern.*") + len("key")
    c.kpool_max = c.kpool_bytes() + 10
    c.bind(VH, "q", "h", "", {"name": "value!"})      # 4 + 6 bytes: the pool's last
    x = c.exchanges[(VH, "h")]
    for fn, args in ((c.bind, (VH, "r", "h", "", {"n": ""})), (c.bind_exchange, (VH, "t", "h", "", {"n": ""}))):
        with pytest.raises(ControlError) as e:
            fn(*args)
        assert e.value.code == 506 and len(x.hbindings) == 1 and not x.hxbindings
    c.bind(VH, "r", "h", "", {"x-only": "free", "x-match": "any"})      # no pairs: no bytes
    assert c.kpool_bytes() == c.kpool_max and len(x.hbindings) == 2
    c.kpool_max = None
    c.hop_qmax = 2
    with pytest.raises(ControlError) as e:
        c.bind(VH, "s", "h", "", {})
    assert e.value.code == 506 and len(x.hbindings) == 2
    c.bind(VH, "r", "h", "k2", {"more": "rows of a bound queue"})
    assert len(x.hbindings) == 3
