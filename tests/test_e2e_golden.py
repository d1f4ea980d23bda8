"""Exchange-to-exchange bindings on the CPU: the golden model's closure against a brute-force
oracle, the bind-time bounds and refusals, route_host, the Exchange.Bind / Exchange.Unbind
conversation of the GPU-path server on the golden plane (and the same script against the
host broker), and golden clusters of 2 and 3 ranks against the single-plane oracle."""

import pytest

from chanamq_amd.engine.control import ControlError
from chanamq_amd.engine.golden import GoldenDataPlane
from chanamq_amd.models.matcher import topic_match
from chanamq_amd.parallel.cluster import LocalCluster
from chanamq_amd.protocol import constants as C
from e2e_scenarios import (SCENARIOS, apply_e2e, deliveries, publishes, run_e2e, sc_hundred, sc_random_graph,
                           sp_e2e_sharded, topology)

VH = "AMQ.DEFAULT"
SMALL = dict(c_max=64, chpc=8, q_max=64, x_max=64, cons_max=256, ucap=256, deliver_cap=4096)


def golden(**kw):
    cfg = dict(SMALL, default_queue_capacity=1 << 12, ring_pool=1 << 20)
    cfg.update(kw)
    return GoldenDataPlane(**cfg)


# ---------------------------------------------------------------- brute-force oracle
def oracle_route(topo, exchange, key):
    """Queue names a publish entering at ``exchange`` reaches: plain sets and topic_match.
    Reachable exchanges are the least fixed point of "an edge of a reached exchange matches
    the key by that exchange's type"; the queues are those bound to any of them by a binding
    that matches the same way."""
    xs, qbinds, xbinds = topo

    def matches(x, pattern):
        if xs[x] == "fanout":
            return True
        if xs[x] == "direct":
            return pattern == key
        return topic_match(pattern, key)
    if exchange not in xs:
        return set()
    reached = {exchange}
    while True:
        more = {dst for dst, src, k in xbinds if src in reached and matches(src, k)} - reached
        if not more:
            break
        reached |= more
    return {q for q, x, k in qbinds if x in reached and matches(x, k)}


def check_routes(dp, pubs):
    topo = topology(dp)
    n_hops = 0
    for ex, key in pubs:
        x = dp.exchanges[(VH, ex)]
        got = dp._route(x, key.encode())
        names = [dp.queue_by_slot[s].name for s in got]
        assert len(names) == len(set(names)), (ex, key, names)          # one copy per queue
        assert set(names) == oracle_route(topo, ex, key), (ex, key)
        assert dp.route_host(x, key.encode()) == got, (ex, key)       # the same list, in the same order
        n_hops += bool(x.xbindings)
    return n_hops


@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_golden_routes_match_oracle(name):
    g = golden()
    steps = SCENARIOS[name](g)
    pubs = publishes(steps)
    assert pubs
    assert check_routes(g, pubs) > 0, "no publish entered at an exchange with edges"


def expected_deliveries(topo, pubs):
    want = {}
    for ex, key in pubs:
        for q in oracle_route(topo, ex, key):
            want.setdefault("c-" + q, []).append(key)
    return want


@pytest.mark.parametrize("name", ["chain_types", "cycle", "diamond", "topic_source", "long_chain", "wide"])
def test_golden_deliveries_match_oracle(name):
    """End to end on the golden plane: every queue's consumer gets exactly the publishes the
    oracle routes to it, in publish order."""
    g = golden()
    steps = SCENARIOS[name](g)
    topo = topology(g)
    got = deliveries(run_e2e(g, steps))
    assert got == expected_deliveries(topo, publishes(steps))


def test_golden_wide_reaches_forty_queues_once():
    g = golden()
    steps = SCENARIOS["wide"](g)
    got = deliveries(run_e2e(g, steps))
    n_k = sum(1 for _, k in publishes(steps) if k == "k")
    n_j = sum(1 for _, k in publishes(steps) if k == "j")
    assert len(got) == 40
    for i in range(40):   # the direct branch (w15..w39) matches only "k"; w00..w24 get everything
        assert len(got[f"c-w{i:02d}"]) == (n_k + n_j if i < 25 else n_k), i


def test_golden_hundred_queues_behind_a_hop():
    g = golden(q_max=256)
    steps = sc_hundred(g)
    got = deliveries(run_e2e(g, steps))
    assert len(got) == 100 and all(v == ["k", "k"] for v in got.values())


def test_golden_random_graph_matches_oracle():
    g = golden()
    steps = sc_random_graph(g)
    pubs = publishes(steps)
    assert len(pubs) == 200
    assert check_routes(g, pubs) > 50
    assert deliveries(run_e2e(g, steps)) == expected_deliveries(topology(g), pubs)


def test_golden_returns_and_confirms():
    from chanamq_amd.protocol.codec import CommandAssembler, FrameParser
    g = golden()
    outs = run_e2e(g, SCENARIOS["returns"](g))
    fp, ca = FrameParser(), CommandAssembler()
    cmds = [c for o in outs for fr in fp.feed(o["egress"].get(1, b"")) for c in [ca.feed(fr)] if c is not None]
    rets = [(c.method.reply_code, c.method.routing_key) for c in cmds if c.method.name == "basic.return"]
    assert rets == [(312, "nogo"), (313, "go")]
    acks = [c.method for c in cmds if c.method.name == "basic.ack"]
    assert [a.delivery_tag for a in acks] == [4, 6] and not [c for c in cmds if c.method.name == "basic.nack"]
    got = deliveries(outs)
    assert got["c-qt"] == ["go2", "go2"]
    assert got["late"] == ["go"]           # the mandatory "go" was stored; the immediate one was not


def test_unbind_then_delete_between_steps():
    g = golden()
    steps = SCENARIOS["unbind_delete"](g)
    got = deliveries(run_e2e(g, steps))
    assert got == {"c-qb": ["k", "k"], "c-qc": ["k", "k", "k", "k"]}
    assert g.exchanges[(VH, "ua")].xbindings == []


def test_exchange_without_edges_routes_as_before():
    g = golden()
    g.declare_exchange(VH, "p", "topic")
    g.declare_exchange(VH, "src", "fanout")
    for q, pat in (("q2", "a.*"), ("q1", "a.b"), ("q1", "#")):
        g.declare_queue(VH, q)
        g.bind(VH, q, "p", pat)
    x = g.exchanges[(VH, "p")]
    before = g._route(x, b"a.b")
    g.bind_exchange(VH, "p", "src", "")           # p is a destination only: still the plain path
    assert g._route(x, b"a.b") == before == g._route_flat(x, b"a.b")
    assert g._route(g.exchanges[(VH, "src")], b"a.b") == before


# ---------------------------------------------------------------- bounds and refusals
def _refused(code, fn, *args):
    with pytest.raises(ControlError) as e:
        fn(*args)
    assert e.value.code == code, e.value
    return e.value


def _edges(dp):
    return sorted((x.name, s, k) for x in dp.exchanges.values() for s, k in x.xbindings)


def test_default_exchange_and_missing_exchanges_are_refused():
    g = golden()
    g.declare_exchange(VH, "a", "direct")
    for fn in (g.bind_exchange, g.unbind_exchange):
        _refused(C.ACCESS_REFUSED, fn, VH, "", "a", "k")
        _refused(C.ACCESS_REFUSED, fn, VH, "a", "", "k")
        _refused(C.NOT_FOUND, fn, VH, "a", "missing", "k")
        _refused(C.NOT_FOUND, fn, VH, "missing", "a", "k")
    g.ensure_vhost("other")
    g.declare_exchange("other", "b", "direct")
    _refused(C.NOT_FOUND, g.bind_exchange, VH, "b", "a", "k")    # both names resolve in one vhost
    assert _edges(g) == []


def test_duplicate_bind_and_missing_unbind_are_noops():
    g = golden()
    calls = []
    g.routing_changed = lambda: calls.append(1)
    g.declare_exchange(VH, "a", "direct")
    g.declare_exchange(VH, "b", "fanout")
    g.bind_exchange(VH, "b", "a", "k")
    n = len(calls)
    g.bind_exchange(VH, "b", "a", "k")
    g.unbind_exchange(VH, "b", "a", "other")
    assert len(calls) == n and _edges(g) == [("a", g.exchanges[(VH, "b")].slot, b"k")]
    g.unbind_exchange(VH, "b", "a", "k")
    assert len(calls) == n + 1 and _edges(g) == []


def test_delete_exchange_drops_edges_both_ways_and_if_unused_counts_edges():
    g = golden()
    for n in ("a", "b", "c"):
        g.declare_exchange(VH, n, "fanout")
    g.bind_exchange(VH, "b", "a", "")
    g.bind_exchange(VH, "c", "b", "")
    g.bind_exchange(VH, "a", "c", "")
    _refused(C.PRECONDITION_FAILED, g.delete_exchange, VH, "b", True)   # an outgoing edge is use
    g.delete_exchange(VH, "b")
    assert _edges(g) == [("c", g.exchanges[(VH, "a")].slot, b"")]
    g.declare_exchange(VH, "b2", "fanout")            # takes b's slot: nothing points at it
    assert g._route(g.exchanges[(VH, "c")], b"x") == []
    g.unbind_exchange(VH, "a", "c", "")
    g.delete_exchange(VH, "c", if_unused=True)


def test_exchange_slot_bound():
    g = golden(x_max=4096)
    g.declare_exchange(VH, "low", "fanout")
    n = 0
    while g.declare_exchange(VH, f"fill{n}", "fanout") < g.hop_xslots:
        n += 1
    high = f"fill{n}"
    assert g.exchanges[(VH, high)].slot == g.hop_xslots == 2048
    _refused(C.RESOURCE_ERROR, g.bind_exchange, VH, high, "low", "")
    _refused(C.RESOURCE_ERROR, g.bind_exchange, VH, "low", high, "")
    assert _edges(g) == []
    g.bind_exchange(VH, f"fill{n - 1}", "low", "")    # slot 2047 takes part


def test_distinct_queue_bound_on_exchange_bind_and_queue_bind():
    g = golden(q_max=2048, ring_pool=1 << 22, default_queue_capacity=16)
    assert g.hop_qmax >= 256
    cap = g.hop_qmax
    for n in ("front", "mid", "leaf", "big"):
        g.declare_exchange(VH, n, "fanout")
    for i in range(cap + 1):
        g.declare_queue(VH, f"q{i}")
    for i in range(cap):
        g.bind(VH, f"q{i}", "leaf", "")
        g.bind(VH, f"q{i}", "big", "")
    g.bind(VH, f"q{cap}", "big", "")                  # big alone: cap + 1 queues, no edge, fine
    g.bind_exchange(VH, "mid", "front", "")
    g.bind_exchange(VH, "leaf", "mid", "")            # exactly the cap behind front and mid
    g.bind(VH, "q0", "mid", "again")                  # counted once: still the cap
    _refused(C.RESOURCE_ERROR, g.bind, VH, f"q{cap}", "leaf", "")      # Queue.Bind downstream
    _refused(C.RESOURCE_ERROR, g.bind, VH, f"q{cap}", "front", "")
    assert (g.queues[(VH, f"q{cap}")].slot, b"") not in g.exchanges[(VH, "leaf")].bindings
    _refused(C.RESOURCE_ERROR, g.bind_exchange, VH, "big", "mid", "")  # Exchange.Bind
    _refused(C.RESOURCE_ERROR, g.bind_exchange, VH, "front", "big", "")
    assert len(_edges(g)) == 2
    assert len(g._route(g.exchanges[(VH, "front")], b"x")) == cap


def test_topic_rows_with_edges_count_against_the_topic_table():
    g = golden()
    g.tb_max = 6                                      # the device table's rows (GpuDataPlane: info["tb_max"])
    g.declare_exchange(VH, "t", "topic")
    g.declare_exchange(VH, "h", "headers")
    g.declare_exchange(VH, "d", "direct")
    g.declare_queue(VH, "q")
    for i in range(3):
        g.bind(VH, "q", "t", f"a.{i}")
    g.bind_exchange(VH, "d", "t", "x.*")
    g.bind_exchange(VH, "d", "h", "y.*")
    g.bind_exchange(VH, "t", "d", "k")                # a direct source takes no topic row
    g.bind_exchange(VH, "d", "h", "z.#")              # row 6
    before = _edges(g)
    _refused(C.RESOURCE_ERROR, g.bind_exchange, VH, "d", "t", "w.*")
    assert _edges(g) == before


# ---------------------------------------------------------------- server conversation (golden plane)
def _script(port, vhost="/"):
    """A front exchange fanned into per-team topic exchanges; returns {queue: [bodies]}
    after each of three phases (all edges, one unbound, a destination deleted)."""
    from chanamq_amd.client import Connection
    c = Connection(port=port, vhost=vhost)
    ch = c.channel()
    ch.exchange_declare("front", "direct")
    ch.exchange_declare("team.a", "topic")
    ch.exchange_declare("team.b", "topic")
    ch.exchange_declare("audit", "fanout")
    queues = {"qa1": ("team.a", "a.*"), "qa2": ("team.a", "#"), "qb": ("team.b", "*.urgent"), "qlog": ("audit", "")}
    for q, (x, k) in queues.items():
        ch.queue_declare(q)
        ch.queue_bind(q, x, k)
    ch.exchange_bind("team.a", "front", "a.urgent")
    ch.exchange_bind("team.b", "front", "a.urgent")
    ch.exchange_bind("team.b", "front", "b.urgent")
    ch.exchange_bind("audit", "team.b", "#")
    ch.exchange_bind("audit", "team.a", "a.*")
    ch.exchange_bind("audit", "team.a", "a.*")        # duplicate
    ch._send("exchange.bind", destination="audit", source="front", routing_key="direct.audit", nowait=True)
    ch.exchange_unbind("audit", "front", "never.bound")
    cc = c.channel()
    for q in queues:
        cc.basic_consume(q, q, no_ack=True)
    keys = ["a.urgent", "b.urgent", "direct.audit", "nobody"]

    def phase(tag, want):
        for k in keys:
            ch.basic_publish("front", k, f"{tag}:{k}".encode())
        got = {}
        for d in cc.consume_n(want):
            got.setdefault(d.method.consumer_tag, []).append(d.body.decode())
        return {q: sorted(v) for q, v in got.items()}
    out = [phase("p1", 7)]     # a.urgent -> qa1 qa2 qb qlog; b.urgent -> qb qlog; direct.audit -> qlog
    ch.exchange_unbind("team.b", "front", "a.urgent")
    out.append(phase("p2", 6))
    ch.exchange_delete("audit")
    out.append(phase("p3", 3))
    c.close()
    return out


EXPECTED = [
    {"qa1": ["p1:a.urgent"], "qa2": ["p1:a.urgent"], "qb": ["p1:a.urgent", "p1:b.urgent"],
     "qlog": ["p1:a.urgent", "p1:b.urgent", "p1:direct.audit"]},
    {"qa1": ["p2:a.urgent"], "qa2": ["p2:a.urgent"], "qb": ["p2:b.urgent"],
     "qlog": ["p2:a.urgent", "p2:b.urgent", "p2:direct.audit"]},
    {"qa1": ["p3:a.urgent"], "qa2": ["p3:a.urgent"], "qb": ["p3:b.urgent"]},
]


def _serve(plane, io, **kw):
    from chanamq_amd.server.gpu_broker import GpuBroker
    return GpuBroker(plane, idle_step_ms=1.0, io=io, ingress_bytes=8 << 20, **kw).start()


def conversation(b):
    """Capability flag, the script, and the refusals, against a GpuBroker with the feature on."""
    from chanamq_amd.client import ChannelClosed, Connection
    c = Connection(port=b.port, vhost="/")
    assert c.server_properties["capabilities"]["exchange_exchange_bindings"] is True
    ch = c.channel()
    ch.exchange_declare("only", "direct")
    for args, code in ((("", "only", "k"), 403), (("only", "", "k"), 403), (("only", "missing", "k"), 404),
                       (("missing", "only", "k"), 404)):
        ch = c.channel()
        with pytest.raises(ChannelClosed) as e:
            ch.exchange_bind(*args)
        assert e.value.code == code, args
    c.close()
    assert _script(b.port) == EXPECTED


@pytest.mark.parametrize("io", ["native", "python"])
def test_server_conversation_on_golden_plane(io):
    b = _serve(golden(), io, exchange_bindings=True)
    try:
        conversation(b)
    finally:
        b.stop()


def test_server_off_by_default_keeps_540_and_the_flag():
    from chanamq_amd.client import Connection, ConnectionClosed
    b = _serve(golden(), "python")
    try:
        c = Connection(port=b.port, vhost="/")
        assert c.server_properties["capabilities"]["exchange_exchange_bindings"] is False
        with pytest.raises(ConnectionClosed) as e:
            c.channel().exchange_bind("amq.direct", "amq.fanout", "k")
        assert e.value.code == 540
    finally:
        b.stop()


def test_host_broker_yields_the_same_message_sets(tmp_path):
    """The same script against the host broker (csrc/core): chains of at most 8 hops."""
    from chanamq_amd.broker import load
    hb = load().Broker({"port": 0, "host": "127.0.0.1", "heartbeat": 0, "data_dir": str(tmp_path / "data")})
    hb.start()
    try:
        assert _script(hb.port, vhost="/") == EXPECTED
    finally:
        hb.stop()


def test_config_key_reaches_the_broker(tmp_path):
    from chanamq_amd.utils.config import Config
    assert Config.load([], {}).gpu_config()[1]["exchange_bindings"] is False
    f = tmp_path / "on.conf"
    f.write_text("chana.mq.gpu.exchange-bindings = true\n")
    for single in (True, False):
        assert Config.load([str(f)], {}).gpu_config(single=single)[1]["exchange_bindings"] is True


def test_control_log_replicates_edges():
    from chanamq_amd.parallel.control_log import REPLICATED
    assert {"bind_exchange", "unbind_exchange"} <= REPLICATED


# ---------------------------------------------------------------- sharded: golden cluster vs one plane
def run_single_e2e(spec, world, make=golden):
    remap = {c: (r % world) * 16 + c for c, r in spec.rank_of.items()}
    back = {v: k for k, v in remap.items()}
    dp = make(c_max=1024)
    apply_e2e(dp, spec, conn_map=remap)
    out = []
    for k, st in enumerate(spec.steps):
        eg = dp.step({remap[c]: b for c, b in st.items()}, now_ms=1000 + k)["egress"]
        out.append({back[c]: b for c, b in eg.items()})
    return out


def run_cluster_e2e(spec, world, make):
    from sharded_scenarios import split_inputs
    cl = LocalCluster(make, world)
    for r in range(world):
        apply_e2e(cl[r], spec, rank=r, world=world)
    outs = []
    for k, st in enumerate(spec.steps):
        res = cl.step(split_inputs(spec, st, world), now_ms=1000 + k)
        merged = {}
        for r in res:
            eg = r["egress"] if isinstance(r, dict) else r.egress
            assert not set(eg) & set(merged)
            merged.update(eg)
        outs.append(merged)
    return cl, outs


def assert_cluster_matches(single, clus):
    assert len(single) == len(clus)
    for k, (a, b) in enumerate(zip(single, clus)):
        assert set(a) == set(b), (k, sorted(a), sorted(b))
        for c in a:
            assert a[c] == b[c], (k, c)
    assert any(single), "scenario produced no egress"


@pytest.mark.parametrize("world", [2, 3])
def test_golden_cluster_matches_single_plane(world):
    single = run_single_e2e(sp_e2e_sharded(), world)
    cl, clus = run_cluster_e2e(sp_e2e_sharded(), world, lambda **kw: golden(**kw))
    assert_cluster_matches(single, clus)
    # the scenario covers what it claims: from rank 0, "one.x" has one remote queue and no
    # local one (the MF_ONEQ case), "many" several remote queues and more than 8 local ones
    p0 = cl[0]
    owners = lambda key: [p0.queue_by_slot[s].owner for s in p0._route(p0.exchanges[(VH, "sa")], key)]
    assert owners(b"one.x") == [1]
    assert sum(1 for o in owners(b"many") if o != 0) >= 2 and sum(1 for o in owners(b"many") if o == 0) > 8


def test_edge_table_capacity_is_refused():
    """hopx_max (engine config ``hopx_max``, like fan_max): the edges of all fanout sources,
    and of all direct sources, that the device lists hold."""
    g = golden()
    g.hopx_max = 2
    for n, t in (("f", "fanout"), ("d", "direct"), ("x1", "fanout"), ("x2", "fanout"), ("x3", "fanout")):
        g.declare_exchange(VH, n, t)
    for src in ("f", "d"):
        g.bind_exchange(VH, "x1", src, "k")
        g.bind_exchange(VH, "x2", src, "k")
        before = _edges(g)
        _refused(C.RESOURCE_ERROR, g.bind_exchange, VH, "x3", src, "k")
        assert _edges(g) == before


# ---------------------------------------------------------------- sharded server over TCP
@pytest.mark.timeout(300)
def test_sharded_server_serves_exchange_bind(tmp_path):
    """Two ranks of the sharded server (golden planes, gloo) with the capability on:
    Exchange.Bind / Unbind go through the control log, are answered once applied on every
    rank (or not at all with nowait), refusals come back as channel errors, and a publish
    on rank 0 crosses an edge into a queue that lives on rank 1."""
    import json
    import os
    import time

    from chanamq_amd.client import ChannelClosed, Connection
    from chanamq_amd.parallel.launch import Launcher
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, PYTHONPATH=os.path.dirname(here))
    ln = Launcher(2, ["-m", "chanamq_amd.server.sharded", "--config", os.path.join(here, "sharded_small.conf"),
                      "--set", "chana.mq.gpu.exchange-bindings=true", "--plane", "golden", "--port", "0",
                      "--info-dir", str(tmp_path)], env=env).start()
    try:
        deadline = time.time() + 120
        while time.time() < deadline and not all((tmp_path / f"rank{r}.json").exists() for r in range(2)):
            assert not ln.poll(), f"rank exited early: {ln.poll()}"
            time.sleep(0.2)
        ports = [json.load(open(tmp_path / f"rank{r}.json"))["port"] for r in range(2)]
        c0, c1 = Connection(port=ports[0], vhost="/"), Connection(port=ports[1], vhost="/")
        assert c0.server_properties["capabilities"]["exchange_exchange_bindings"] is True
        a, b = c0.channel(), c1.channel()
        a.exchange_declare("front", "direct")
        a.exchange_declare("team", "topic")
        b.queue_declare("qb")                       # lives on rank 1
        b.queue_bind("qb", "team", "a.*")
        a.exchange_bind("team", "front", "a.x")     # answered when every rank applied it
        a._send("exchange.bind", destination="team", source="front", routing_key="a.y", nowait=True)
        a.exchange_bind("team", "front", "a.x")     # duplicate
        b.basic_consume("qb", "cb", no_ack=True)
        for k in ("a.x", "nope", "a.y"):
            a.basic_publish("front", k, k.encode())
        assert [d.body for d in b.consume_n(2)] == [b"a.x", b"a.y"]
        b.exchange_unbind("team", "front", "a.x")   # from the other rank
        for k in ("a.x", "a.y"):
            a.basic_publish("front", k, b"again " + k.encode())
        assert [d.body for d in b.consume_n(1)] == [b"again a.y"]
        for args, code in ((("", "front", "k"), 403), (("team", "missing", "k"), 404)):
            ch = c0.channel()
            with pytest.raises(ChannelClosed) as e:
                ch.exchange_bind(*args)
            assert e.value.code == code, args
        c0.close()
        c1.close()
    finally:
        ln.stop()
