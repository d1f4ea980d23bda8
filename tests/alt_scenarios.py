"""Alternate-exchange scenarios (``alternate_exchange=True``), shared by the golden model's tests
(tests/test_golden_alt.py) and the HIP data plane's (tests/test_gpu_alt.py).

A scenario is a function ``(dp) -> Rec``.  It declares its topology on ``dp`` and publishes
through the ``Rec``, naming for every publish what has to become of it: the queues it reaches, the
alternates its walk takes, the reply code of a return.  These are written down by the scenario,
from the rule in CHANGES.md "Alternate exchanges on the GPU path" -- never taken from
``route_closure``.  ``check`` holds a run to that record: every consumer's deliveries in publish
order, the returns, ``n_alt`` / ``n_unroutable`` / ``n_unknown_exchange`` / ``n_returns`` per step
and the depth of the queues nobody consumes.  The GPU tests then compare the run byte for byte
with the golden model's."""

import random
from collections import defaultdict, namedtuple

from chanamq_amd.protocol.codec import Method, render_command
from dp_scenarios import NOW, VH
from route_scenarios import body_of, observe

ALT = "alternate-exchange"
COUNTERS = ("n_alt", "n_unroutable", "n_unknown_exchange", "n_deliv", "n_returns",
            "n_dl_expired", "n_dl_unrouted", "n_dl_cycle", "n_dl_pending", "n_expired")
SHARED = tuple(c for c in COUNTERS if c != "n_returns")   # (the golden model counts no returns: its wire shows them)
Pub = namedtuple("Pub", "step body queues ret")


class Rec:
    """The scenario's record.  Publisher: connection 1, channel 1.  A queue declared with
    ``consume=True`` gets an auto-ack consumer ``c-<queue>``, eight to a connection from 20 up."""

    def __init__(self, dp, now_step_ms=0):
        self.dp, self.now_step_ms = dp, now_step_ms
        self.steps, self.pubs, self.counters = [], [], []
        self.cons, self.idle = set(), set()
        self.also = {}     # deliveries that are no publish's own: {consumer tag: [bodies]} (dead letters)
        self._cur, self._ops, self._cnt = [], [], defaultdict(int)
        dp.open_connection(1, VH)
        dp.open_channel(1, 1)

    # -- topology
    def x(self, name, type_="direct", alt=None, **kw):
        return self.dp.declare_exchange(VH, name, type_, arguments={ALT: alt} if alt is not None else None, **kw)

    def q(self, name, binds=(), consume=True, **kw):
        """Queue ``name`` bound by ``binds``: [(exchange, key)] or [(exchange, key, arguments)]."""
        self.dp.declare_queue(VH, name, **kw)
        for b in binds:
            self.dp.bind(VH, name, *b)
        if consume:
            n = len(self.cons)
            conn = 20 + n // 8
            if n % 8 == 0:
                self.dp.open_connection(conn, VH)
                self.dp.open_channel(conn, 1)
            self.dp.consume(conn, 1, VH, name, "c-" + name, no_ack=True)
            self.cons.add(name)
        else:
            self.idle.add(name)

    def edge(self, src, dst, key=""):
        self.dp.bind_exchange(VH, dst, src, key)

    def slot(self, name):
        return self.dp.exchanges[(VH, name)].slot

    # -- traffic
    def pub(self, ex, key, to=(), alt=0, ret=0, mandatory=False, immediate=False, props=None, unknown=False):
        """One publish; ``to``: the queues it has to reach, ``alt``: the alternates its walk takes,
        ``ret``: the reply code it comes back with (0: it does not)."""
        body = body_of(len(self.pubs), 24 + len(self.pubs) % 5)
        m = Method("basic.publish", exchange=ex, routing_key=key, mandatory=mandatory, immediate=immediate)
        self._cur.append(render_command(1, m, props or {}, body))
        self.pubs.append(Pub(len(self.steps), body, () if ret == 313 else tuple(to), ret))
        self._cnt["n_alt"] += alt
        self._cnt["n_unroutable"] += (not to and not unknown and ret != 313)   # (313: routed, nobody consumes)
        self._cnt["n_unknown_exchange"] += bool(unknown)
        self._cnt["n_returns"] += bool(ret)

    def op(self, name, *args, **kw):
        """A control call applied before the step being recorded."""
        self._ops.append((name, args, kw))

    def end(self, n=1):
        """Close the step (and ``n - 1`` empty ones after it)."""
        for _ in range(n):
            inp = {1: b"".join(self._cur)} if self._cur else {}
            if self._ops:
                inp["__ops__"] = self._ops
            self.steps.append(inp)
            self.counters.append(dict(self._cnt))
            self._cur, self._ops, self._cnt = [], [], defaultdict(int)
        return self


def run_alt(dp, rec):
    outs = []
    for k, inp in enumerate(rec.steps):
        inp = dict(inp)
        for name, args, kw in inp.pop("__ops__", []):
            getattr(dp, name)(*args, **kw)
        r = dp.step(inp, now_ms=NOW + rec.now_step_ms * k)
        if isinstance(r, dict):
            eg, ctrl, ev, segs, tx, cnt = r["egress"], r["ctrl"], r["events"], r["segs"], r.get("txbuf", []), r["counters"]
        else:
            eg, ctrl, ev, segs, tx, cnt = r.egress, r.ctrl, r.events, [s[:4] for s in r.segs], r.txbuf, r.counters
        outs.append(dict(egress=eg, ctrl=sorted(ctrl), events=sorted(ev), gets=[], txbuf=sorted(tx),
                         segs=sorted((s[0], s[1], s[2], s[3]) for s in segs),
                         counters={c: int(cnt[c]) for c in COUNTERS if c in cnt},
                         depth={q.name: dp.message_count(q.slot) for q in dp.queues.values()}))
    return outs


def check(rec, outs, returns_counted=True):
    """The run against the scenario's record.  ``returns_counted``: the plane keeps n_returns."""
    seen = observe(outs)
    got = defaultdict(list)
    for s in seen:
        if s.kind == "deliver":
            got[s.ctag].append(bytes(s.body))
    want = defaultdict(list)
    for p in rec.pubs:
        for q in p.queues:
            if q in rec.cons:
                want["c-" + q].append(p.body)
    for t, bodies in rec.also.items():
        want[t] += bodies
    assert {t: v for t, v in got.items() if v} == dict(want), "deliveries: not the publishes the scenario routes"
    rets = [(s.step, s.code, bytes(s.body)) for s in seen if s.kind == "return"]
    assert rets == [(p.step, p.ret, p.body) for p in rec.pubs if p.ret], "returns"
    for k, named in enumerate(rec.counters):
        for c in ("n_alt", "n_unroutable", "n_unknown_exchange") + (("n_returns",) if returns_counted else ()):
            g = outs[k]["counters"].get(c, 0)
            assert g == named.get(c, 0), f"step {k}: {c} = {g}, expected {named.get(c, 0)}"
    for q in rec.idle:
        n = sum(1 for p in rec.pubs if q in p.queues)
        assert outs[-1]["depth"][q] == n, f"queue {q}: depth {outs[-1]['depth'][q]}, expected {n}"
    for q in rec.cons:
        assert outs[-1]["depth"][q] == 0, f"queue {q} is not drained"


def totals(outs, c):
    return sum(o["counters"].get(c, 0) for o in outs)


# ---------------------------------------------------------------- scenarios
def sc_types(dp):
    """A direct, a fanout without bindings, a topic and a headers-match exchange, each with the
    fanout ``ca`` as alternate: a miss is caught, a hit is not.  (A fanout without bindings cannot
    hit: ``f2``, with one, stands in for it.)"""
    r = Rec(dp)
    r.x("ca", "fanout")
    r.x("d", "direct", alt="ca")
    r.x("f", "fanout", alt="ca")
    r.x("f2", "fanout", alt="ca")
    r.x("t", "topic", alt="ca")
    r.x("h", "headers", alt="ca")
    r.q("qca", [("ca", "")])
    r.q("qd", [("d", "k")])
    r.q("qf2", [("f2", "")])
    r.q("qt", [("t", "a.*")])
    r.q("qh", [("h", "", {"x-match": "all", "kind": "order"})])
    hit, miss = {"headers": {"kind": "order"}}, {"headers": {"kind": "other"}}
    r.pub("d", "nope", ["qca"], alt=1)
    r.pub("d", "k", ["qd"])
    r.pub("f", "any", ["qca"], alt=1)
    r.pub("f2", "any", ["qf2"])
    r.pub("t", "b.c", ["qca"], alt=1)
    r.pub("t", "a.c", ["qt"])
    r.pub("h", "", ["qca"], alt=1, props=miss)
    r.pub("h", "", ["qca"], alt=1)           # no headers at all
    r.pub("h", "", ["qh"], props=hit)
    return r.end(2)


def sc_chain(dp):
    """x -> a1 -> a2 -> a3 as alternates, a3 without one."""
    r = Rec(dp)
    r.x("a3", "direct")
    r.x("a2", "direct", alt="a3")
    r.x("a1", "topic", alt="a2")
    r.x("x", "direct", alt="a1")
    r.q("q1", [("a1", "mid.*")])
    r.q("q2", [("a2", "two")])
    r.q("q3", [("a3", "deep")])
    r.pub("x", "deep", ["q3"], alt=3)                           # caught at the third level
    r.pub("x", "nothing", alt=3, ret=312, mandatory=True)       # falls through the whole chain: one unroutable
    r.pub("x", "mid.a", ["q1"], alt=1, mandatory=True)          # caught on the way: no return
    r.pub("x", "two", ["q2"], alt=2, mandatory=True)
    r.pub("x", "nothing", alt=3)                                # not mandatory: dropped
    return r.end(2)


def sc_cycle(dp):
    """x and y name each other and both miss: the walk ends, the publish is unroutable.  ``s`` names
    itself."""
    r = Rec(dp)
    r.x("x", "direct", alt="y")
    r.x("y", "direct", alt="x")
    r.x("s", "topic", alt="s")
    r.q("qy", [("y", "ky")])
    r.q("qs", [("s", "ks")])
    r.pub("x", "none", alt=1, ret=312, mandatory=True)   # x takes y; y's alternate x is visited: not taken
    r.pub("y", "none", alt=1)
    r.pub("x", "ky", ["qy"], alt=1)
    r.pub("s", "none", ret=312, mandatory=True)          # visited before its own alternate is looked at
    r.pub("s", "ks", ["qs"])
    return r.end(2)


def sc_per_exchange(dp):
    """The rule is per exchange, not per publish: x binds q1 and has an edge to y, y matches nothing
    and has alternate z: the message reaches q1 and z's queues.  Conversely c hits a queue and has
    an alternate, which is not taken."""
    r = Rec(dp)
    r.x("z", "fanout")
    r.x("x", "fanout")
    r.x("y", "direct", alt="z")
    r.x("c", "direct", alt="z")
    r.edge("x", "y")
    r.q("q1", [("x", "")])
    r.q("qz1", [("z", "")])
    r.q("qz2", [("z", "")])
    r.q("qc", [("c", "k")])
    r.pub("x", "any", ["q1", "qz1", "qz2"], alt=1)
    r.pub("c", "k", ["qc"])
    r.pub("c", "j", ["qz1", "qz2"], alt=1)
    return r.end(2)


def sc_edge_only(dp):
    """x's only hit is an edge to y, which matches nothing and has no alternate: x had a
    destination, so its alternate is not taken and the publish is unroutable."""
    r = Rec(dp)
    r.x("a", "fanout")
    r.x("y", "direct")
    r.x("x", "direct", alt="a")
    r.edge("x", "y", "k")
    r.q("qa", [("a", "")])
    r.pub("x", "k", ret=312, mandatory=True)
    r.pub("x", "other", ["qa"], alt=1, mandatory=True)
    r.pub("x", "k")
    return r.end(2)


def sc_listed_hit(dp):
    """Matches count before the walk's deduplication: l1, late in the walk, hits only q1, which l0
    listed; l2 hits only an edge back to l0, which is visited.  Neither takes its alternate."""
    r = Rec(dp)
    r.x("la", "fanout")
    r.x("l0", "fanout")
    r.x("l1", "fanout", alt="la")
    r.x("l2", "fanout", alt="la")
    assert r.slot("l0") < r.slot("l1") < r.slot("l2")
    r.edge("l0", "l1")
    r.edge("l0", "l2")
    r.edge("l2", "l0")
    r.q("q1", [("l0", ""), ("l1", "")])
    r.q("qa", [("la", "")])
    r.pub("l0", "k", ["q1"])
    r.pub("l2", "k", ["q1"])
    r.pub("l1", "k", ["q1"])
    return r.end(2)


def sc_slots(dp):
    """More than 70 exchanges: alternates in slots below 32, in 32..63 and above 64 (lanes 0, 1 and
    2 of the walk's visited / pending registers), and two alternates pending at once."""
    r = Rec(dp)
    n = [0]

    def fill(upto):
        while r.x(f"fill{n[0]}", "fanout") < upto - 1:
            n[0] += 1
        n[0] += 1
    r.x("a0", "fanout")
    fill(40)
    r.x("a1", "fanout")
    fill(70)
    r.x("a2", "fanout")
    assert r.slot("a0") < 32 <= r.slot("a1") < 64 <= r.slot("a2") and len(dp.exchanges) >= 70
    for i in range(3):
        r.x(f"e{i}", "direct", alt=f"a{i}")
        r.q(f"s{i}", [(f"a{i}", "")])
    # top -> m1, m2 (both miss); m1 names a2 (slot above 64), m2 names a0 (below 32): both are
    # pending once m2 is matched, and a0 is matched first
    r.x("top", "fanout")
    r.x("m1", "direct", alt="a2")
    r.x("m2", "direct", alt="a0")
    r.edge("top", "m1")
    r.edge("top", "m2")
    for i in range(3):
        r.pub(f"e{i}", "k", [f"s{i}"], alt=1)
    r.pub("top", "k", ["s0", "s2"], alt=2)
    r.pub("m2", "k", ["s0"], alt=1)
    return r.end(2)


WIDE = (9, 65, 130)


def sc_wide(dp):
    """Alternate fanouts with 9, 65 and 130 queues: a walk past PUB_QC into hop_q, and more than
    one and more than two 64-lane batches in hop_finish."""
    r = Rec(dp)
    for n in WIDE:
        r.x(f"w{n}", "fanout")
        r.x(f"d{n}", "direct", alt=f"w{n}")
    for i in range(max(WIDE)):
        r.q(f"q{i:03d}", [(f"w{n}", "") for n in WIDE if i < n], capacity=64)
    for n in WIDE + WIDE:
        r.pub(f"d{n}", "k", [f"q{i:03d}" for i in range(n)], alt=1)
    return r.end(2)


def sc_unresolved(dp):
    """The alternate is named but absent (dropped), then declared (caught), then deleted (dropped)."""
    r = Rec(dp)
    r.x("x", "direct", alt="late")
    r.q("ql")
    r.pub("x", "k", ret=312, mandatory=True)
    r.pub("x", "k")
    r.end()
    r.op("declare_exchange", VH, "late", "fanout")
    r.op("bind", VH, "ql", "late", "")
    r.pub("x", "k", ["ql"], alt=1, mandatory=True)
    r.pub("x", "k", ["ql"], alt=1)
    r.end()
    r.op("delete_exchange", VH, "late")
    r.pub("x", "k", ret=312, mandatory=True)
    r.pub("x", "k")
    return r.end(2)


def sc_immediate(dp):
    """313 is decided by the consumers of the final set: an immediate publish caught by a queue
    without consumers is returned; with a consumer it is delivered."""
    r = Rec(dp)
    r.x("a1", "fanout")
    r.x("a2", "fanout")
    r.x("x1", "direct", alt="a1")
    r.x("x2", "direct", alt="a2")
    r.q("idle", [("a1", "")], consume=False)
    r.q("busy", [("a2", "")])
    r.pub("x1", "k", alt=1, ret=313, immediate=True)
    r.pub("x2", "k", ["busy"], alt=1, immediate=True)
    r.pub("x1", "k", ["idle"], alt=1)                    # not immediate: kept for a later consumer
    return r.end(2)


def sc_group16(dp):
    """One block's 16 publishes: the plain path, an edge walk, a caught publish, a fall-through and
    an unknown exchange side by side (the block's waves share hop_list)."""
    r = Rec(dp)
    r.x("plain", "direct")
    r.x("ca", "fanout")
    r.x("hop", "fanout")
    r.x("leaf", "topic")
    r.x("caught", "direct", alt="ca")
    r.x("hole", "direct", alt="hole2")
    r.x("hole2", "direct")
    r.edge("hop", "leaf")
    r.q("qp", [("plain", "k")])
    r.q("qca", [("ca", "")])
    r.q("ql", [("leaf", "#")])
    r.q("qc", [("caught", "k")])
    for i in range(16):
        kind = i % 7
        if kind == 0:
            r.pub("plain", "k", ["qp"])
        elif kind == 1:
            r.pub("hop", "a.b", ["ql"])
        elif kind == 2:
            r.pub("caught", "miss", ["qca"], alt=1)
        elif kind == 3:
            r.pub("hole", "miss", alt=1, ret=312, mandatory=True)
        elif kind == 4:
            r.pub("caught", "k", ["qc"])
        elif kind == 5:
            r.pub("plain", "miss")
        else:
            r.pub("nowhere", "k", unknown=True)     # (the plane reports 404 and routes on)
    assert len(r.pubs) == 16
    return r.end(2)


def sc_dead_alt(dp):
    """``dead_letter=True, x_death=True``: the dead-letter exchange matches nothing and its
    alternate takes the dead letter.  ``src``, behind the alternate, is the queue the message
    expired in: the history bans it (n_dl_cycle); t0 and t1 get the message."""
    r = Rec(dp, now_step_ms=1000)
    r.x("dla", "fanout")
    r.x("dlx", "direct", alt="dla")
    r.q("t0", [("dla", "")])
    r.q("t1", [("dla", ""), ("dlx", "elsewhere")])
    r.q("src", [("dla", "")], consume=False, ttl_ms=500, dead_letter_exchange="dlx")
    for _ in range(3):
        r.pub("", "src", ["src"])
    r.end(5)
    # step 1: the three expire and join the dead list; step 2: the dead pass routes them
    r.idle.discard("src")
    r.also = {"c-t0": [p.body for p in r.pubs], "c-t1": [p.body for p in r.pubs]}
    r.counters[2]["n_alt"] = 3
    return r


def brute_route(xs, qbinds, xbinds, alts, ex, key):
    """Brute-force worklist router of the random graph: ``xs`` {exchange: type}, ``qbinds``
    [(queue, exchange, key)], ``xbinds`` [(destination, source, key)], ``alts`` {exchange:
    alternate}.  Returns (queue names, alternates taken)."""
    from chanamq_amd.models.matcher import topic_match

    def hit(x, pattern):
        return xs[x] == "fanout" or (pattern == key if xs[x] == "direct" else topic_match(pattern, key))
    order = list(xs)     # (declaration order is slot order)
    done, work, queues, taken = [], [ex], set(), 0
    while work:
        cur = min(work, key=order.index)
        work.remove(cur)
        done.append(cur)
        qs = {q for q, x, k in qbinds if x == cur and hit(cur, k)}
        ds = {d for d, s, k in xbinds if s == cur and hit(cur, k)}
        queues |= qs
        work += [d for d in ds if d not in done and d not in work]
        a = alts.get(cur)
        if not qs and not ds and a in xs and a not in done:
            taken += 1
            if a not in work:
                work.append(a)
    return queues, taken


def sc_random_graph(dp, seed=23):
    """12 exchanges of every type (headers routes as topic: headers_match is off here) with random
    bindings, edges and alternates, 160 publishes over every entry exchange, each routed by
    ``brute_route``."""
    rnd = random.Random(seed)
    r = Rec(dp)
    words = ["a", "b", "cc"]
    types = ["direct", "fanout", "topic", "headers"]
    names = [f"g{i}" for i in range(12)]
    xs, alts = {}, {}
    for i, x in enumerate(names):
        xs[x] = types[i % 4] if i < 8 else rnd.choice(types)
        if rnd.random() < 0.6:
            alts[x] = rnd.choice(names + ["absent"])
        r.x(x, xs[x], alt=alts.get(x))
    assert [r.slot(x) for x in names] == sorted(r.slot(x) for x in names)

    def key_for(x):
        n = rnd.randint(1, 3)
        pool = words if xs[x] in ("direct", "fanout") else words + ["*", "#"]
        return ".".join(rnd.choice(pool) for _ in range(n))
    qbinds, xbinds = [], []
    for i in range(24):
        q = f"r{i:02d}"
        bs = []
        for _ in range(rnd.randint(1, 2)):
            x = rnd.choice(names[:9])     # (g9 .. g11 bind nothing: reached, they miss)
            bs.append((x, key_for(x)))
        r.q(q, bs, capacity=1024)
        qbinds += [(q, x, k) for x, k in bs]
    for _ in range(10):
        src, dst = rnd.choice(names), rnd.choice(names)
        k = key_for(src)
        r.edge(src, dst, k)
        xbinds.append((dst, src, k))
    n_alt = 0
    for i in range(160):
        ex, key = rnd.choice(names), ".".join(rnd.choice(words) for _ in range(rnd.randint(1, 3)))
        qs, taken = brute_route(xs, qbinds, xbinds, alts, ex, key)
        n_alt += taken
        r.pub(ex, key, sorted(qs), alt=taken)
        if i == 79:
            r.end()
    assert n_alt > 20, "the graph takes too few alternates to test anything"
    return r.end(2)


Scenario = namedtuple("Scenario", "fn cfg flags")
BIG = dict(q_max=256, x_max=128)
SCENARIOS = {
    "types": Scenario(sc_types, {}, dict(headers_match=True)),
    "chain": Scenario(sc_chain, {}, {}),
    "cycle": Scenario(sc_cycle, {}, {}),
    "per_exchange": Scenario(sc_per_exchange, {}, {}),
    "edge_only": Scenario(sc_edge_only, {}, {}),
    "listed_hit": Scenario(sc_listed_hit, {}, {}),
    "slots": Scenario(sc_slots, BIG, {}),
    "wide": Scenario(sc_wide, BIG, {}),
    "unresolved": Scenario(sc_unresolved, {}, {}),
    "immediate": Scenario(sc_immediate, {}, {}),
    "group16": Scenario(sc_group16, {}, {}),
    "dead_alt": Scenario(sc_dead_alt, {}, dict(dead_letter=True, x_death=True)),
    "random_graph": Scenario(sc_random_graph, {}, {}),
}


def golden_plane(cfg, alternate_exchange=True, **flags):
    from chanamq_amd.engine.golden import GoldenDataPlane
    from consumer_scenarios import GOLDEN_KEYS
    kw = {k: cfg[k] for k in GOLDEN_KEYS + ("ring_pool", "deliv_max", "egress_cap") if k in cfg}
    return GoldenDataPlane(alternate_exchange=alternate_exchange, **kw, **flags)


def gpu_plane(cfg, graph=True, alternate_exchange=True, **flags):
    from chanamq_amd.engine.dataplane import GpuDataPlane
    return GpuDataPlane(graph=graph, alternate_exchange=alternate_exchange, **dict(cfg, **flags))


# ---------------------------------------------------------------- sharded (sharded_scenarios.Spec)
def sp_alt_sharded():
    """Alternates whose queues sit on other ranks.  From rank 0's publisher: ``one`` misses ``sx``
    and is caught by a single queue on rank 1 (the record travels with its queue); ``miss`` at ``sy``
    is caught by a fanout with thirteen queues, eleven of them local and two on rank 1 at world 2,
    where both callers run it (an owner of 2 folds onto rank 0), so pass 1 copies the walk's list;
    ``k`` hits locally and takes no alternate."""
    from e2e_scenarios import stream
    from sharded_scenarios import Spec
    s = Spec()
    s.xbinds = []
    s.alts = [("sa1", "fanout", None), ("sa2", "fanout", None), ("sx", "direct", "sa1"), ("sy", "topic", "sa2")]
    owners = {"r1": 1, "loc": 0}
    s.binds += [("r1", "sa1", ""), ("loc", "sx", "k")]
    for i in range(10):
        owners[f"n{i}"] = 0
        s.binds.append((f"n{i}", "sa2", ""))
    for i, o in enumerate((1, 2, 1)):
        owners[f"m{i}"] = o
        s.binds.append((f"m{i}", "sa2", ""))
    for q, o in owners.items():
        s.queues.append((q, o, 1 << 10))
    for o in range(3):
        s.conn(o, 10 + o, 1)
    for q, o in owners.items():
        s.consumers.append((10 + o, 1, q, "c-" + q, True))
    s.conn(0, 1, 1)
    s.conn(1, 2, 1)
    s.steps = [{1: stream([("sx", "one"), ("sy", "miss"), ("sx", "k"), ("sx", "one")], seed=40),
                2: stream([("sy", "miss.too"), ("sx", "k")], seed=41)},
               {1: stream([("sy", "x"), ("sx", "two")], seed=42)}, {}, {}]
    return s


def with_alts(make, spec):
    """``make`` for test_e2e_golden's run_single_e2e / run_cluster_e2e: the plane with the spec's
    exchanges declared (``spec.alts``: name, type, alternate), the same on every rank."""
    def made(**kw):
        dp = make(**kw)
        for name, t, alt in spec.alts:
            dp.declare_exchange(VH, name, t, arguments={ALT: alt} if alt else None)
        return dp
    return made
