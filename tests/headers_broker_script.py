"""Conversations with a server about headers exchanges, through the AMQP test client: shared by
tests/test_headers_broker.py (GpuBroker on the golden plane), tests/test_gpu_headers_broker.py
(GpuBroker on the HIP plane) and tests/test_headers_host_agreement.py (the native host
broker).  Every expected message set is written out by hand from the rule (x-match all / any,
x- names ignored, void = presence, integers and booleans compared as their text)."""

from decimal import Decimal

from chanamq_amd.protocol.codec import Typed

QUEUES = ["q_all", "q_any", "q_void", "q_int", "q_zero"]
BINDS = {"q_all": {"x-match": "all", "region": "eu", "tier": "gold"},
         "q_any": {"x-match": "any", "region": "eu", "tier": "gold"},
         "q_void": {"flag": None}, "q_int": {"n": "5", "ok": "true"}, "q_zero": {}}
MESSAGES = [("m0", {"region": "eu", "tier": "gold"}), ("m1", {"region": "eu"}), ("m2", {"region": "us", "flag": "x"}),
            ("m3", {"n": Typed("b", 5), "ok": True}), ("m4", {"n": Typed("l", 5), "ok": False}), ("m5", None),
            ("m6", {"flag": None, "tier": "gold"})]
EXPECTED = {"q_all": ["m0"], "q_any": ["m0", "m1", "m6"], "q_void": ["m2", "m6"], "q_int": ["m3"],
            "q_zero": ["m0", "m1", "m2", "m3", "m4", "m5", "m6"]}
# option off: every binding has the key "" and so has every publish: all of them match
EXPECTED_OFF = {q: [m for m, _ in MESSAGES] for q in QUEUES}


def collect(cc, want):
    got = {}
    for d in cc.consume_n(want):
        got.setdefault(d.method.consumer_tag, []).append(d.body.decode())
    return {q: sorted(v) for q, v in got.items()}


def publish_all(ch, x, tag=""):
    for name, hdrs in MESSAGES:
        ch.basic_publish(x, "", (tag + name).encode(), {} if hdrs is None else {"headers": hdrs})


def script(port, x="hx", vhost="/"):
    """Bind with arguments, publish with headers, consume: {queue: [bodies]}."""
    from chanamq_amd.client import Connection
    c = Connection(port=port, vhost=vhost)
    ch = c.channel()
    ch.exchange_declare(x, "headers")
    for q in QUEUES:
        ch.queue_declare(q)
        ch.queue_bind(q, x, "", BINDS[q])
    cc = c.channel()
    for q in QUEUES:
        cc.basic_consume(q, q, no_ack=True)
    publish_all(ch, x)
    out = collect(cc, sum(map(len, EXPECTED.values())))
    c.close()
    return out


def unbind_script(port, x="hu", vhost="/"):
    """Two bindings of one queue and key that differ in their arguments only; a duplicate
    bind; an unbind that names other arguments (nothing goes), then one of the two."""
    from chanamq_amd.client import Connection
    c = Connection(port=port, vhost=vhost)
    ch = c.channel()
    ch.exchange_declare(x, "headers")
    ch.queue_declare("u")
    ch.queue_bind("u", x, "k", {"a": "1"})
    ch.queue_bind("u", x, "k", {"b": "2"})
    ch.queue_bind("u", x, "k", {"a": Typed("I", 1)})        # the same binding as the first: a no-op
    cc = c.channel()
    cc.basic_consume("u", "u", no_ack=True)
    msgs = [("a", {"a": "1"}), ("b", {"b": "2"}), ("ab", {"a": "1", "b": "2"}), ("n", {"c": "3"})]

    def phase(tag, want):
        for name, h in msgs:
            ch.basic_publish(x, "", f"{tag}:{name}".encode(), {"headers": h})
        return sorted(d.body.decode() for d in cc.consume_n(want))
    out = [phase("p1", 3)]
    ch.queue_unbind("u", x, "k", {"a": "2"})
    out.append(phase("p2", 3))
    ch.queue_unbind("u", x, "k", {"a": "1"})
    out.append(phase("p3", 2))
    ch.queue_unbind("u", x, "k", {"b": "2"})
    ch.queue_bind("u", x, "k", {"c": "3"})
    out.append(phase("p4", 1))
    c.close()
    return out


UNBIND_EXPECTED = [["p1:a", "p1:ab", "p1:b"], ["p2:a", "p2:ab", "p2:b"], ["p3:ab", "p3:b"], ["p4:n"]]

DURABLE_BINDS = [{"x-match": "any", "a": "1", "v": None}, {"d": 2.5}, {"D": Decimal("1.50"), "n": Typed("s", -3)}]
DURABLE_MSGS = [("v", {"v": "anything"}), ("a", {"a": Typed("B", 1)}), ("d", {"d": 2.5}), ("df", {"d": Typed("f", 2.5)}),
                ("Dn", {"D": Decimal("1.50"), "n": "-3"}), ("D", {"D": Decimal("1.5"), "n": "-3"}), ("none", {"z": "z"})]
DURABLE_EXPECTED = ["Dn", "a", "d", "v"]


def durable_setup(port):
    from chanamq_amd.client import Connection
    c = Connection(port=port, vhost="/")
    ch = c.channel()
    ch.exchange_declare("dur.h", "headers", durable=True)
    ch.queue_declare("dur.q", durable=True)
    for a in DURABLE_BINDS:
        ch.queue_bind("dur.q", "dur.h", "k", a)
    c.close()


def durable_check(port, tag):
    from chanamq_amd.client import Connection
    c = Connection(port=port, vhost="/")
    ch = c.channel()
    ch.queue_declare("dur.q", durable=True, passive=True)
    cc = c.channel()
    cc.basic_consume("dur.q", "dur.q", no_ack=True)
    for name, h in DURABLE_MSGS:
        ch.basic_publish("dur.h", "", f"{tag}:{name}".encode(), {"headers": h})
    got = sorted(d.body.decode() for d in cc.consume_n(len(DURABLE_EXPECTED)))
    c.close()
    return got
