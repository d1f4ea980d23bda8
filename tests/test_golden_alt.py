"""Alternate exchanges on the CPU: every scenario of tests/alt_scenarios.py on the golden model,
judged by the scenarios' own record; the control plane's rules (406, the no-op redeclare, 506 with
the state unchanged, the flag off); route_host; recovery of a durable exchange with its alternate;
the replicated declare; a 2-rank golden cluster against the single-plane oracle.
tests/test_gpu_alt.py holds the HIP data plane to the same record and to byte equality with this
model."""

import pytest

from alt_scenarios import ALT, SCENARIOS, check, golden_plane, run_alt, sp_alt_sharded, totals, with_alts
from chanamq_amd.engine.control import ControlError, ControlState
from chanamq_amd.engine.golden import GoldenDataPlane
from chanamq_amd.protocol import constants as C
from gpu_cfg import CFG
from test_e2e_golden import assert_cluster_matches, golden, run_cluster_e2e, run_single_e2e

VH = "AMQ.DEFAULT"


@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_golden_keeps_the_rule(name):
    sc = SCENARIOS[name]
    g = golden_plane(dict(CFG, **sc.cfg), **sc.flags)
    rec = sc.fn(g)
    outs = run_alt(g, rec)
    check(rec, outs, returns_counted=False)
    if name == "dead_alt":
        dead_alt_outcome(rec, outs)


def dead_alt_outcome(rec, outs):
    """The three messages expire in ``src``; each dead letter misses ``dlx``, is taken by ``dla``,
    is refused by ``src`` (its own history) and reaches t0 and t1."""
    assert totals(outs, "n_dl_expired") == 3 and totals(outs, "n_dl_cycle") == 3 and totals(outs, "n_dl_unrouted") == 0
    assert totals(outs, "n_alt") == 3
    assert outs[-1]["depth"]["src"] == 0 and outs[-1]["counters"].get("n_dl_pending", 0) == 0


def test_flag_is_a_keyword_of_every_plane():
    for cls in (ControlState, GoldenDataPlane):
        assert cls(alternate_exchange=True).alternate_exchange and not cls().alternate_exchange


def test_config_key():
    from chanamq_amd.utils.config import Config
    c = Config.load([], {}, env=False)
    plane, broker = c.gpu_config()
    assert "alternate_exchange" not in plane and broker["alternate_exchange"] is False
    c.set("chana.mq.gpu.alternate-exchange", True)
    for single in (True, False):
        plane, broker = c.gpu_config(single=single)
        assert plane["alternate_exchange"] is True and broker["alternate_exchange"] is True


def test_broker_flag_needs_the_planes():
    from chanamq_amd.server.gpu_broker import GpuBroker
    with pytest.raises(ValueError, match="alternate_exchange"):
        GpuBroker(golden(), io="python", alternate_exchange=True)


# ---------------------------------------------------------------- control plane
def on(**kw):
    return golden(alternate_exchange=True, **kw)


def refused(code, fn, *a, **kw):
    with pytest.raises(ControlError) as e:
        fn(*a, **kw)
    assert e.value.code == code, e.value
    return e.value


def state(g):
    return (sorted((x.name, x.slot, x.alt, tuple(x.bindings), tuple(x.xbindings)) for x in g.exchanges.values()),
            list(g._free_x), sorted(g.exch_by_slot))


def test_invalid_argument_is_406_and_changes_nothing():
    g = on()
    before = state(g)
    for bad in (5, True, 1.5, ["ae"], {"a": 1}, "x" * 256, b"y" * 256):
        e = refused(C.PRECONDITION_FAILED, g.declare_exchange, VH, "x", "direct", arguments={ALT: bad})
        assert (e.class_id, e.method_id) == (40, 10)
    assert state(g) == before
    g.declare_exchange(VH, "x", "direct", arguments={ALT: "a" * 255})
    g.declare_exchange(VH, "y", "direct", arguments={ALT: b"bytes-name"})
    assert g.exchanges[(VH, "x")].alt == "a" * 255 and g.exchanges[(VH, "y")].alt == "bytes-name"


def test_redeclare_rules():
    g = on()
    s = g.declare_exchange(VH, "x", "direct", arguments={ALT: "ae"})
    g.declare_exchange(VH, "plain", "direct")
    before = state(g)
    assert g.declare_exchange(VH, "x", "direct", arguments={ALT: "ae"}) == s       # the same: fine
    assert g.declare_exchange(VH, "x", "direct") == s                               # none named: the no-op
    assert g.declare_exchange(VH, "x", "direct", arguments={"other": 1}) == s
    refused(C.PRECONDITION_FAILED, g.declare_exchange, VH, "x", "direct", arguments={ALT: "other"})
    refused(C.PRECONDITION_FAILED, g.declare_exchange, VH, "plain", "direct", arguments={ALT: "ae"})
    assert g.declare_exchange(VH, "x", "direct", arguments={ALT: "other"}, passive=True) == s   # passive: not compared
    assert state(g) == before and g.exchanges[(VH, "x")].alt == "ae"


def test_flag_off_ignores_the_argument():
    g = golden()
    g.declare_exchange(VH, "ae", "fanout")
    s = g.declare_exchange(VH, "x", "direct", arguments={ALT: "ae"})
    assert g.declare_exchange(VH, "x", "direct", arguments={ALT: "other"}) == s     # the unconditional no-op
    assert g.declare_exchange(VH, "y", "direct", arguments={ALT: 5}) >= 0           # not even validated
    x = g.exchanges[(VH, "x")]
    assert x.alt is None and x.arguments == {ALT: "ae"}
    g.declare_queue(VH, "q")
    g.bind(VH, "q", "ae", "")
    assert g._route(x, b"k") == [] == g.route_host(x, b"k") and g.alt_taken == 0


def test_default_exchange_and_self_are_legal_alternates():
    g = on()
    g.declare_queue(VH, "q")
    g.declare_exchange(VH, "x", "direct", arguments={ALT: ""})
    g.declare_exchange(VH, "s", "direct", arguments={ALT: "s"})
    assert g._route(g.exchanges[(VH, "x")], b"q") == [g.queues[(VH, "q")].slot]
    assert g._route(g.exchanges[(VH, "x")], b"nobody") == []
    assert g._route(g.exchanges[(VH, "s")], b"q") == []


def reach_setup(g, n):
    """``big`` binds n queues; q_extra is one more, bound nowhere yet."""
    g.declare_exchange(VH, "big", "fanout")
    for i in range(n):
        g.declare_queue(VH, f"q{i}")
        g.bind(VH, f"q{i}", "big", "")
    g.declare_queue(VH, "extra")


def test_506_declare_whose_alternate_is_over_the_reach():
    g = on()
    g.hop_qmax = 4
    reach_setup(g, 5)                  # no exchange has edges: five queues behind big are fine
    before = state(g)
    e = refused(C.RESOURCE_ERROR, g.declare_exchange, VH, "x", "direct", arguments={ALT: "big"})
    assert (e.class_id, e.method_id) == (40, 10)
    assert state(g) == before and (VH, "x") not in g.exchanges
    slot = g._free_x[-1]
    assert g.declare_exchange(VH, "x", "direct") == slot     # the slot went back on the free list


def test_506_declare_of_the_named_exchange():
    g = on()
    g.hop_qmax = 4
    for i in range(3):
        g.declare_queue(VH, f"own{i}")
    g.declare_exchange(VH, "x", "fanout", arguments={ALT: "late"})   # absent: nothing to check yet
    for i in range(3):
        g.bind(VH, f"own{i}", "x", "")
    g.declare_exchange(VH, "chain", "fanout")
    for i in range(2):
        g.declare_queue(VH, f"c{i}")
        g.bind(VH, f"c{i}", "chain", "")
    before = state(g)
    # "late" resolves x's alternate; with its own alternate "chain" x would reach 3 + 2 queues
    refused(C.RESOURCE_ERROR, g.declare_exchange, VH, "late", "direct", arguments={ALT: "chain"})
    assert state(g) == before
    g.declare_exchange(VH, "late", "direct")                 # without the chain: 3 queues
    assert g._alt_of(g.exchanges[(VH, "x")]) is g.exchanges[(VH, "late")]


def test_506_bind_downstream_of_an_alternate():
    g = on()
    g.hop_qmax = 4
    reach_setup(g, 4)
    g.declare_exchange(VH, "x", "direct", arguments={ALT: "big"})    # exactly the cap
    before = state(g)
    refused(C.RESOURCE_ERROR, g.bind, VH, "extra", "big", "")        # downstream of x's alternate
    refused(C.RESOURCE_ERROR, g.bind, VH, "extra", "x", "k")         # and x's own
    g.declare_exchange(VH, "leaf", "fanout")
    g.bind(VH, "extra", "leaf", "")
    refused(C.RESOURCE_ERROR, g.bind_exchange, VH, "leaf", "big", "")
    # (leaf is new; the refused calls changed nothing:)
    assert [r for r in state(g)[0] if r[0] != "leaf"] == before[0]
    assert (g.queues[(VH, "extra")].slot, b"") not in g.exchanges[(VH, "big")].bindings
    assert g.exchanges[(VH, "x")].bindings == [] and g.exchanges[(VH, "big")].xbindings == []
    g.bind(VH, "q0", "x", "again")                                   # counted once: still the cap


def test_flag_off_accepts_the_same_declares():
    g = golden()
    g.hop_qmax = 4
    reach_setup(g, 5)
    g.declare_exchange(VH, "x", "direct", arguments={ALT: "big"})
    g.bind(VH, "extra", "big", "")
    assert g._route(g.exchanges[(VH, "x")], b"k") == []


def test_slot_bound():
    g = on(x_max=4096)
    g.declare_exchange(VH, "low", "fanout")
    n = 0
    while g.declare_exchange(VH, f"fill{n}", "fanout") < g.hop_xslots - 1:
        n += 1
    before = state(g)
    refused(C.RESOURCE_ERROR, g.declare_exchange, VH, "high", "direct", arguments={ALT: "low"})   # slot 2048
    assert state(g) == before
    g.declare_exchange(VH, "named-later", "direct", arguments={ALT: "high"})    # (slot 2048, unresolved: fine)
    refused(C.RESOURCE_ERROR, g.declare_exchange, VH, "high", "fanout")         # resolving it is not


def test_route_host_follows_alternates():
    g = on(headers_match=True)
    rec = SCENARIOS["chain"].fn(g)
    x = g.exchanges[(VH, "x")]
    slot = lambda q: g.queues[(VH, q)].slot
    assert g.route_host(x, b"deep") == [slot("q3")] == g._route(x, b"deep")
    assert g.route_host(x, b"mid.a") == [slot("q1")]
    assert g.route_host(x, b"nothing") == []
    assert rec.pubs


def test_durable_exchange_keeps_its_alternate_through_recovery(tmp_path):
    from chanamq_amd.broker import load
    from chanamq_amd.engine.persistence import GpuPersistence
    core = load()

    def node():
        st = core.Store()
        st.open(str(tmp_path / "store"), True)
        g = on(persist=True)
        return g, GpuPersistence(g, st), st
    g, ps, st = node()
    g.declare_exchange(VH, "ae", "fanout", durable=True)
    g.declare_exchange(VH, "front", "direct", durable=True, arguments={ALT: "ae"})
    g.declare_queue(VH, "caught", durable=True)
    g.bind(VH, "caught", "ae", "")
    for x in ("ae", "front"):
        ps.exchange(g.exchanges[(VH, x)])
    ps.queue(g.queues[(VH, "caught")])
    ps.bind(VH, "caught", "ae", "")
    ps.commit()
    st.close()
    g2, ps2, st2 = node()
    ps2.recover()
    x = g2.exchanges[(VH, "front")]
    assert x.alt == "ae" and x.durable
    assert g2._route(x, b"nobody") == [g2.queues[(VH, "caught")].slot]
    st2.close()


def test_control_log_carries_the_argument():
    """A sharded declare: the argument travels in the keywords of the control log's
    ``declare_exchange`` op, through its JSON form, and every replica that applies the op keeps the
    alternate and routes by it."""
    import json

    from chanamq_amd.parallel.control_log import REPLICATED, ControlLog
    assert "declare_exchange" in REPLICATED
    a, b = ControlState(alternate_exchange=True), ControlState(alternate_exchange=True)
    log = ControlLog(a, None)
    log.submit("declare_exchange", VH, "ae", "fanout", durable=True, auto_delete=False, internal=False, arguments={})
    log.submit("declare_exchange", VH, "x", "direct", durable=True, auto_delete=False, internal=False,
               arguments={ALT: "ae", "other": 5})
    log.submit("declare_queue", VH, "caught")
    log.submit("bind", VH, "caught", "ae", "", None)
    ops = json.loads(json.dumps(log.outbox))
    assert ops[1][2]["arguments"] == {ALT: "ae", "other": 5}
    for p in (a, b):
        for op, args, kw in ops:
            getattr(p, op)(*args, **kw)
        x = p.exchanges[(VH, "x")]
        assert x.alt == "ae" and x.durable and x.arguments == {ALT: "ae", "other": 5}
        assert p.route_host(x, b"nobody") == [p.queues[(VH, "caught")].slot]
    # a replica refuses what the rule refuses: the op's error is the control plane's 406
    for p in (a, b):
        refused(C.PRECONDITION_FAILED, p.declare_exchange, VH, "x", "direct", arguments={ALT: "elsewhere"})


def test_sharded_broker_refuses_before_it_submits():
    """GpuBroker._replicated (a sharded node's Exchange.Declare): a value that is no string and a
    redeclare naming another alternate are 406 before anything reaches the control log; a fresh
    declare, the same alternate again and a redeclare without the argument are submitted, with
    the arguments in the op."""
    from types import SimpleNamespace

    from chanamq_amd.protocol.codec import Method
    from chanamq_amd.server.gpu_broker import GpuBroker
    plane = on()
    plane.open_connection(3, VH)

    class Node:
        ops = []

        def submit(self, op, *args, **kw):
            self.ops.append((op, args, kw))
            return len(self.ops)
    node = Node()
    broker = SimpleNamespace(plane=plane, node=node, _deferred={}, _send=lambda *a: None)
    conn = SimpleNamespace(id=3, last_queue={})

    def declare(name, arguments, **kw):
        m = Method("exchange.declare", exchange=name, type="direct", passive=False, durable=False, auto_delete=False,
                   internal=False, nowait=False, arguments=arguments, **kw)
        return GpuBroker._replicated(broker, conn, 1, m)
    assert declare("front", {ALT: "ae"}) == "deferred"
    assert node.ops == [("declare_exchange", (VH, "front", "direct"),
                         dict(durable=False, auto_delete=False, internal=False, arguments={ALT: "ae"}))]
    plane.declare_exchange(*node.ops[0][1], **node.ops[0][2])        # (the log applies it)
    assert declare("front", {ALT: "ae"}) == "deferred" and declare("front", {}) == "deferred"
    n = len(node.ops)
    for bad in ({ALT: "other"}, {ALT: 5}, {ALT: "x" * 256}):
        e = refused(C.PRECONDITION_FAILED, declare, "front", bad)
        assert (e.class_id, e.method_id) == (40, 10)
    refused(C.PRECONDITION_FAILED, declare, "fresh", {ALT: ["no", "string"]})
    assert len(node.ops) == n and broker._deferred.keys() == set(range(1, n + 1))
    # with the flag off the same declares are submitted unexamined, as before
    broker.plane = golden()
    broker.plane.open_connection(3, VH)
    assert declare("front", {ALT: 5}) == "deferred" and len(node.ops) == n + 1


def test_default_exchange_as_alternate_counts_one_queue():
    """The default exchange binds every queue of its vhost, by name: as an alternate it adds one
    queue at most to any walk, and is counted so -- queues declared later, which grow it without a
    check, never make a bind upstream fail."""
    g = on()
    g.hop_qmax = 4
    g.declare_exchange(VH, "x", "direct", arguments={ALT: ""})
    for i in range(8):                       # more queues in the vhost than the walk holds
        g.declare_queue(VH, f"q{i}")
    for i in range(3):
        g.bind(VH, f"q{i}", "x", f"k{i}")      # 3 of x's own + 1 through the default exchange: the cap
    refused(C.RESOURCE_ERROR, g.bind, VH, "q3", "x", "k3")
    g.declare_exchange(VH, "y", "direct", arguments={ALT: ""})       # a declare naming "" is not refused either
    x = g.exchanges[(VH, "x")]
    slot = lambda q: g.queues[(VH, q)].slot
    assert g._route(x, b"q7") == [slot("q7")] and g._route(x, b"k1") == [slot("q1")] and g._route(x, b"none") == []


# ---------------------------------------------------------------- sharded: golden cluster vs one plane
def test_golden_cluster_matches_single_plane():
    make = lambda **kw: on(**kw)
    single = run_single_e2e(sp_alt_sharded(), 2, with_alts(make, sp_alt_sharded()))
    cl, clus = run_cluster_e2e(sp_alt_sharded(), 2, with_alts(make, sp_alt_sharded()))
    assert_cluster_matches(single, clus)
    # what the scenario claims: from rank 0, "one" is caught by one remote queue and "miss" by
    # remote queues and more than eight local ones, through alternates only
    p0 = cl[0]
    owners = lambda x, key: [p0.queue_by_slot[s].owner for s in p0._route(p0.exchanges[(VH, x)], key)]
    assert owners("sx", b"one") == [1] and owners("sx", b"k") == [0]
    assert owners("sy", b"miss").count(0) > 8 and owners("sy", b"miss").count(1) >= 2
