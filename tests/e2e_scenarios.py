"""Exchange-to-exchange binding scenarios in the ``dp_scenarios`` style: each is a function
``(dp) -> list[step inputs]`` run on the golden model and on the HIP data plane.  A step
may carry ``{'__ops__': [(control method name, args)]}``: applied before the step by
``run_e2e`` (the unbind / delete driver).  ``topology`` / ``publishes`` expose what a run
used, as plain data, for the brute-force oracle of tests/test_e2e_golden.py.
"""

import random

from chanamq_amd.engine.traffic import publish_command, publish_stream
from chanamq_amd.protocol.codec import CommandAssembler, FrameParser, Method, render_command
from dp_scenarios import VH, run


def consume_all(dp, queues, conn0=20, per_conn=8):
    """An auto-ack consumer ``c-<queue>`` per queue, ``per_conn`` of them per connection."""
    for i, q in enumerate(queues):
        conn = conn0 + i // per_conn
        if i % per_conn == 0:
            dp.open_connection(conn, VH)
            dp.open_channel(conn, 1)
        dp.consume(conn, 1, VH, q, "c-" + q, no_ack=True)


def publisher(dp, conn=1, ch=1):
    dp.open_connection(conn, VH)
    dp.open_channel(conn, ch)


def stream(pubs, size=40, seed=0, channel=1):
    """Publishes [(exchange, key)] as one byte stream."""
    return b"".join(publish_stream(1, ex, lambda i, k=k: k, size + (j % 3) * 8, channel=channel, seed=seed + j)
                    for j, (ex, k) in enumerate(pubs))


def sc_chain_types(dp):
    """direct -> fanout -> topic, a queue at each level; ``qboth`` is bound at two levels."""
    dp.declare_exchange(VH, "cd", "direct")
    dp.declare_exchange(VH, "cf", "fanout")
    dp.declare_exchange(VH, "ct", "topic")
    for q in ("qd", "qf", "qt", "qboth"):
        dp.declare_queue(VH, q)
    dp.bind(VH, "qd", "cd", "k1")
    dp.bind(VH, "qboth", "cd", "k1")
    dp.bind(VH, "qf", "cf", "")
    dp.bind(VH, "qboth", "cf", "ignored")
    dp.bind(VH, "qt", "ct", "a.*")
    dp.bind_exchange(VH, "cf", "cd", "k1")
    dp.bind_exchange(VH, "cf", "cd", "a.b")
    dp.bind_exchange(VH, "cf", "cd", "k1")     # duplicate: no-op
    dp.bind_exchange(VH, "ct", "cf", "")
    consume_all(dp, ["qd", "qf", "qt", "qboth"])
    publisher(dp)
    keys = ["k1", "a.b", "zz", "a.b.c", "a.x"]
    pubs = [("cd", keys[i % 5]) for i in range(15)] + [("cf", keys[i % 5]) for i in range(5)]
    pubs += [("ct", k) for k in keys]
    return [{1: stream(pubs[:13], seed=1)}, {1: stream(pubs[13:], seed=2)}, {}]


def sc_cycle(dp):
    """A -> B -> A and a self-binding: every exchange is matched once."""
    dp.declare_exchange(VH, "ca", "direct")
    dp.declare_exchange(VH, "cb", "fanout")
    dp.declare_queue(VH, "qa")
    dp.declare_queue(VH, "qb")
    dp.bind(VH, "qa", "ca", "k")
    dp.bind(VH, "qb", "cb", "")
    dp.bind_exchange(VH, "cb", "ca", "k")
    dp.bind_exchange(VH, "ca", "cb", "")
    dp.bind_exchange(VH, "ca", "ca", "k")
    dp.bind_exchange(VH, "cb", "cb", "")
    consume_all(dp, ["qa", "qb"])
    publisher(dp)
    pubs = [(x, k) for x in ("ca", "cb") for k in ("k", "x")] * 4
    return [{1: stream(pubs, seed=3)}, {}]


def sc_diamond(dp):
    """A -> B, A -> C, B -> D, C -> D: D's queue gets one copy."""
    dp.declare_exchange(VH, "da", "fanout")
    dp.declare_exchange(VH, "db", "direct")
    dp.declare_exchange(VH, "dc", "topic")
    dp.declare_exchange(VH, "dd", "fanout")
    for q, x, k in (("qb", "db", "k"), ("qc", "dc", "*"), ("qd", "dd", "")):
        dp.declare_queue(VH, q)
        dp.bind(VH, q, x, k)
    dp.bind_exchange(VH, "db", "da", "")
    dp.bind_exchange(VH, "dc", "da", "")
    dp.bind_exchange(VH, "dd", "db", "k")
    dp.bind_exchange(VH, "dd", "dc", "#")
    consume_all(dp, ["qb", "qc", "qd"])
    publisher(dp)
    pubs = [("da", k) for k in ("k", "j", "k.k", "")] * 3 + [("db", "k"), ("dc", "k"), ("db", "j")]
    return [{1: stream(pubs, seed=4)}, {}]


NINE = "w1.w2.w3.w4.w5.w6.w7.w8.w9"


def sc_topic_source(dp):
    """Edges out of a topic exchange: '*' and '#', a pattern only the full matcher decides,
    two patterns to one destination that both match, and a key of 9 words."""
    dp.declare_exchange(VH, "ts", "topic")
    dsts = {"t1": [("a.*"), ("*.b")], "t2": ["#.z"], "t3": ["a.#"], "t4": ["w1.*.*.*.*.*.*.*.w9", "a.*.c.#.z"]}
    for i, (x, pats) in enumerate(dsts.items()):
        dp.declare_exchange(VH, x, ("fanout", "direct", "topic", "headers")[i])
        for pat in pats:
            dp.bind_exchange(VH, x, "ts", pat)
    for q, x, k in (("q1", "t1", ""), ("q2", "t2", "a.z"), ("q3", "t3", "a.*"), ("q4", "t4", "#"),
                    ("qs", "ts", "a.b"), ("qs", "ts", "*.b"), ("q9", "ts", NINE)):
        dp.declare_queue(VH, q)
        dp.bind(VH, q, x, k)
    consume_all(dp, ["q1", "q2", "q3", "q4", "qs", "q9"])
    publisher(dp)
    keys = ["a.b", "a.c", "x.b", "a.z", "q.r.z", "a", "a.b.c.z", "a.b.c.d.e.z", NINE, "z", "", "a..b",
            "w1.w2.w3.w4.w5.w6.w7.w8.w8"]
    return [{1: stream([("ts", k) for k in keys] * 2, seed=5)}, {}]


def sc_long_chain(dp):
    """10 exchanges in a row (the host broker stops following at depth 8; the GPU path does not)."""
    for i in range(10):
        dp.declare_exchange(VH, f"l{i}", ("direct", "fanout", "topic")[i % 3])
    for i in range(9):
        dp.bind_exchange(VH, f"l{i + 1}", f"l{i}", "k")
    for q, x in (("q4", "l4"), ("q9", "l9")):
        dp.declare_queue(VH, q)
        dp.bind(VH, q, x, "k")
    consume_all(dp, ["q4", "q9"])
    publisher(dp)
    pubs = [("l0", "k"), ("l0", "j"), ("l3", "k"), ("l5", "k"), ("l9", "k")] * 3
    return [{1: stream(pubs, seed=6)}, {}]


def sc_wide(dp, n_pubs=24):
    """40 distinct queues through two branches that share 10: more than 8 local queues, so
    pass 1 copies the walk's list."""
    dp.declare_exchange(VH, "wa", "fanout")
    dp.declare_exchange(VH, "wb", "fanout")
    dp.declare_exchange(VH, "wc", "direct")
    dp.bind_exchange(VH, "wb", "wa", "")
    dp.bind_exchange(VH, "wc", "wa", "")
    qs = [f"w{i:02d}" for i in range(40)]
    for i, q in enumerate(qs):
        dp.declare_queue(VH, q)
        if i < 25:
            dp.bind(VH, q, "wb", "")
        if i >= 15:
            dp.bind(VH, q, "wc", "k")
    consume_all(dp, qs)
    publisher(dp)
    pubs = [("wa", "k" if i % 4 else "j") for i in range(n_pubs)]
    return [{1: stream(pubs[:n_pubs // 2], seed=7)}, {1: stream(pubs[n_pubs // 2:], seed=8)}, {}]


def sc_returns(dp):
    """Mandatory publish whose only edge does not match -> 312; immediate with no consumer
    downstream -> 313; with one -> delivered; all on a confirm channel."""
    dp.declare_exchange(VH, "rr", "direct")
    dp.declare_exchange(VH, "rs", "fanout")
    dp.declare_exchange(VH, "rt", "fanout")
    dp.bind_exchange(VH, "rs", "rr", "go")
    dp.bind_exchange(VH, "rt", "rr", "go2")
    dp.declare_queue(VH, "qs")
    dp.declare_queue(VH, "qt")
    dp.bind(VH, "qs", "rs", "")
    dp.bind(VH, "qt", "rt", "")
    consume_all(dp, ["qt"])
    publisher(dp)
    dp.confirm_select(1, 1)
    cmds = []
    for i, (key, mand, imm) in enumerate([("nogo", True, False), ("go", False, True), ("go2", False, True),
                                          ("go", True, False), ("nogo", False, False), ("go2", True, True)]):
        m = Method("basic.publish", exchange="rr", routing_key=key, mandatory=mand, immediate=imm)
        cmds.append(render_command(1, m, {"delivery_mode": 1}, bytes([65 + i]) * (33 + i)))
    return [{1: b"".join(cmds[:4])}, {1: b"".join(cmds[4:])}, {"__consume__": [(30, 1, "qs", "late")]}, {}]


def sc_unbind_delete(dp):
    """An edge unbound, then a destination exchange deleted, between steps."""
    dp.declare_exchange(VH, "ua", "direct")
    dp.declare_exchange(VH, "ub", "fanout")
    dp.declare_exchange(VH, "uc", "fanout")
    dp.declare_queue(VH, "qb")
    dp.declare_queue(VH, "qc")
    dp.bind(VH, "qb", "ub", "")
    dp.bind(VH, "qc", "uc", "")
    dp.bind_exchange(VH, "ub", "ua", "k")
    dp.bind_exchange(VH, "uc", "ua", "k")
    consume_all(dp, ["qb", "qc"])
    publisher(dp)
    pubs = [("ua", "k"), ("ua", "j"), ("ua", "k")]
    return [{1: stream(pubs, seed=9)},
            {"__ops__": [("unbind_exchange", (VH, "ub", "ua", "k")), ("unbind_exchange", (VH, "ub", "ua", "never"))],
             1: stream(pubs, seed=10)},
            {"__ops__": [("delete_exchange", (VH, "uc"))], 1: stream(pubs, seed=11)}, {}]


def sc_hundred(dp):
    """100 queues behind a fanout hop (needs q_max >= 128): emit batches past 64 lanes."""
    dp.declare_exchange(VH, "ha", "direct")
    dp.declare_exchange(VH, "hb", "fanout")
    dp.bind_exchange(VH, "hb", "ha", "k")
    qs = [f"h{i:03d}" for i in range(100)]
    for q in qs:
        dp.declare_queue(VH, q, capacity=64)
        dp.bind(VH, q, "hb", "")
    consume_all(dp, qs, conn0=10, per_conn=4)
    publisher(dp)
    return [{1: stream([("ha", "k"), ("ha", "j"), ("ha", "k")], seed=12)}, {}]


SCENARIOS = {"chain_types": sc_chain_types, "cycle": sc_cycle, "diamond": sc_diamond, "topic_source": sc_topic_source,
             "long_chain": sc_long_chain, "wide": sc_wide, "returns": sc_returns, "unbind_delete": sc_unbind_delete}


def sc_random_graph(dp, seed=11):
    """12 exchanges of mixed types, 30 queues, random queue bindings and edges (cycles and
    self-bindings included), 200 keys over every entry exchange."""
    rnd = random.Random(seed)
    words = ["a", "b", "cc"]
    types = ["direct", "fanout", "topic", "headers"]
    xs = [f"g{i}" for i in range(12)]
    for i, x in enumerate(xs):
        dp.declare_exchange(VH, x, types[i % 4] if i < 8 else rnd.choice(types))
    qs = [f"r{i:02d}" for i in range(30)]
    for q in qs:
        dp.declare_queue(VH, q, capacity=1024)

    def key_for(x):
        t = dp.exchanges[(VH, x)].type
        n = rnd.randint(1, 3)
        if t in ("direct", "fanout"):
            return ".".join(rnd.choice(words) for _ in range(n))
        return ".".join(rnd.choice(words + ["*", "#"]) for _ in range(n))
    for q in qs:
        for _ in range(rnd.randint(1, 2)):
            x = rnd.choice(xs)
            dp.bind(VH, q, x, key_for(x))
    for _ in range(22):
        src, dst = rnd.choice(xs), rnd.choice(xs)
        dp.bind_exchange(VH, dst, src, key_for(src))
    consume_all(dp, qs, conn0=20, per_conn=8)
    publisher(dp)
    pubs = [(rnd.choice(xs), ".".join(rnd.choice(words) for _ in range(rnd.randint(1, 3)))) for _ in range(200)]
    return [{1: stream(pubs[:100], size=32, seed=13)}, {1: stream(pubs[100:], size=32, seed=14)}, {}]


def run_e2e(dp, steps):
    """``dp_scenarios.run`` step by step, with the ``__ops__`` control calls applied first."""
    outs = []
    for inp in steps:
        inp = dict(inp)
        for name, args in inp.pop("__ops__", []):
            getattr(dp, name)(*args)
        outs += run(dp, [inp])
    return outs


def assert_same(og, od):
    """Byte-identical step outputs (the comparison of test_gpu_matches_golden)."""
    assert len(og) == len(od)
    for k, (a, b) in enumerate(zip(og, od)):
        for f in ("segs", "ctrl", "events", "gets", "txbuf"):
            assert a[f] == b[f], f"step {k} {f}"
        assert sorted(a["egress"]) == sorted(b["egress"]), f"step {k} egress conns"
        for c in a["egress"]:
            assert a["egress"][c] == b["egress"][c], f"step {k} conn {c} egress differs"


def publishes(steps):
    """[(exchange, routing key)] of every publish in the steps' inputs, in order."""
    out = []
    for inp in steps:
        for conn, data in inp.items():
            if isinstance(conn, int):
                fp, ca = FrameParser(), CommandAssembler()
                for fr in fp.feed(data):
                    c = ca.feed(fr)
                    if c is not None and c.method is not None and c.method.name == "basic.publish":
                        out.append((c.method.exchange, c.method.routing_key))
    return out


def deliveries(outs):
    """{consumer tag: [routing key]} of every Basic.Deliver in the runs' egress, in order."""
    got = {}
    parsers = {}
    for o in outs:
        for conn, data in sorted(o["egress"].items()):
            fp, ca = parsers.setdefault(conn, (FrameParser(), CommandAssembler()))
            for fr in fp.feed(data):
                c = ca.feed(fr)
                if c is not None and c.method is not None and c.method.name == "basic.deliver":
                    got.setdefault(c.method.consumer_tag, []).append(c.method.routing_key)
    return got


def topology(dp):
    """The control state as plain data: {exchange: type}, [(queue, exchange, key)],
    [(destination, source, key)], names and str keys, for the default vhost."""
    xs = {x.name: x.type for x in dp.exchanges.values() if x.vhost == VH}
    qb = [(dp.queue_by_slot[s].name, x.name, k.decode()) for x in dp.exchanges.values() if x.vhost == VH
          for s, k in x.bindings]
    xb = [(dp.exch_by_slot[s].name, x.name, k.decode()) for x in dp.exchanges.values() if x.vhost == VH
          for s, k in x.xbindings]
    return xs, qb, xb


__all__ = ["SCENARIOS", "sc_hundred", "sc_random_graph", "sc_wide", "run_e2e", "assert_same", "publishes",
           "deliveries", "topology", "publish_command"]


# ---------------------------------------------------------------- sharded (sharded_scenarios.Spec)
def sp_e2e_sharded():
    """The closure's queues owned by different ranks.  From rank 0's publisher: key
    ``one.x`` reaches exactly one queue, on another rank (the record travels with its queue,
    MF_ONEQ); ``many`` reaches 12 local queues (pass 1 copies the walk's list) and several
    remote ones; ``both`` reaches a local and a remote queue through a cycle."""
    from sharded_scenarios import Spec
    s = Spec()
    s.exchanges += [("sa", "direct"), ("sb", "fanout"), ("sc", "topic")]
    s.xbinds = [("sb", "sa", "many"), ("sc", "sa", "one.x"), ("sc", "sa", "both"), ("sa", "sc", "both"),
                ("sc", "sb", "")]
    owners = {}
    for i in range(12):
        owners[f"n{i:02d}"] = 0
        s.binds.append((f"n{i:02d}", "sb", ""))
    for i, o in enumerate((0, 1, 2, 1)):
        owners[f"m{i}"] = o
        s.binds.append((f"m{i}", "sb", ""))
    owners["q1"] = 1
    s.binds.append(("q1", "sc", "one.*"))
    owners["qx"] = 2
    s.binds.append(("qx", "sc", "both"))
    owners["qy"] = 0
    s.binds.append(("qy", "sa", "both"))
    for q, o in owners.items():
        s.queues.append((q, o, 1 << 10))
    for o in range(3):
        s.conn(o, 10 + o, 1)
    for q, o in owners.items():
        s.consumers.append((10 + o, 1, q, "c-" + q, True))
    s.conn(0, 1, 1)
    s.conn(1, 2, 1)
    s.confirms.append((1, 1))
    keys = ["one.x", "many", "both", "none", "one.x", "many"]
    s.steps = [{1: stream([("sa", k) for k in keys], seed=20), 2: stream([("sa", k) for k in keys[:4]], seed=21)},
               {1: stream([("sb", "z"), ("sc", "one.y")], seed=22)}, {}, {}]
    return s


def apply_e2e(dp, spec, rank=None, world=1, conn_map=None):
    from sharded_scenarios import apply
    apply(dp, spec, rank=rank, world=world, conn_map=conn_map)
    for dst, src, key in spec.xbinds:
        dp.bind_exchange(VH, dst, src, key)
