"""Conversations with a ``GpuBroker(priority_queues=True)`` about priority queues, through the AMQP
test client: shared by tests/test_prio_broker.py (golden plane, CPU) and
tests/test_gpu_prio_broker.py (HIP plane).  Every expectation holds however the server cuts the
publishes into steps: nothing is consumed before a confirm says that everything is queued."""

import json

import pytest

from chanamq_amd.protocol.codec import Typed

VH = "AMQ.DEFAULT"
PRIOS = [0, 5, 2, 9, None, 5, 1, 3, 0, 4, 2, 5]      # 9 counts as 5, none as 0
BAD_VALUES = [0, 16, 255, -1, "3", 1.5, True, Typed("l", 1 << 40)]


def publish(ch, q, prios, base=0):
    for i, p in enumerate(prios):
        ch.basic_publish("", q, b"%s-%03d" % (q.encode(), base + i), {"priority": p} if p is not None else None)
    assert ch.wait_for_confirms() is True


def expected(q, prios, P, base=0):
    """The bodies highest priority first, FIFO within one."""
    eff = [(min(p or 0, P), base + i) for i, p in enumerate(prios)]
    return [b"%s-%03d" % (q.encode(), i) for p, i in sorted(eff, key=lambda t: (-t[0], t[1]))]


def rows(b):
    return {r["name"]: r for r in json.loads(b.queues_json())}


def priority_script(b):
    """x-max-priority 5: a mix of priorities in one batch and across batches, read highest first by
    a manual-ack consumer at prefetch 1 and by Basic.Get, with the counts of DeclareOk, GetOk,
    PurgeOk and the admin rows over all priorities."""
    from chanamq_amd.client import Connection
    c = Connection(port=b.port, vhost="/")
    ch = c.channel()
    ch.confirm_select()
    assert ch.queue_declare("work", arguments={"x-max-priority": 5}).message_count == 0
    ch.queue_declare("byget", arguments={"x-max-priority": Typed("s", 5)})
    ch.queue_declare("plain")
    q = b.plane.queues
    assert [q[(VH, n)].max_priority for n in ("work", "byget", "plain")] == [5, 5, None]
    assert len(q[(VH, "work")].lanes) == 6 and len(b.plane.queue_by_slot) == 13
    publish(ch, "work", PRIOS[:7])
    publish(ch, "work", PRIOS[7:], base=7)              # a second batch: still by priority, then by arrival
    publish(ch, "byget", PRIOS)
    publish(ch, "plain", PRIOS)
    n = len(PRIOS)
    assert [ch.queue_declare(x, passive=True).message_count for x in ("work", "byget", "plain")] == [n, n, n]
    assert ch.queue_declare("work", arguments={"x-max-priority": 5}).message_count == n   # an equal redeclare
    assert ch.queue_declare("work").message_count == n                                     # one without the argument
    r = rows(b)
    assert [(r[x]["ready"], r[x]["max_priority"]) for x in ("work", "byget", "plain")] == [(n, 5), (n, 5), (n, None)]
    assert len(r) == 3
    # a consumer with manual acks at prefetch 1: one at a time, highest first
    cc = c.channel()
    cc.basic_qos(prefetch_count=1)
    cc.basic_consume("work", "w", no_ack=False)
    got = []
    for _ in range(n):
        d = cc.consume_n(1)[0]
        got.append(d.body)
        cc.basic_ack(d.delivery_tag)
    assert got == expected("work", PRIOS, 5)
    cc.basic_cancel("w")
    # Basic.Get: the same order, message-count over all priorities
    gc = c.channel()
    got, counts = [], []
    for _ in range(n):
        d = gc.basic_get("byget", no_ack=True)
        got.append(d.body)
        counts.append(d.method.message_count)
    assert got == expected("byget", PRIOS, 5) and counts == list(range(n - 1, -1, -1))
    assert gc.basic_get("byget", no_ack=True) is None
    # a nacked delivery goes back to the front of its own priority, behind nothing lower
    publish(ch, "work", [1, 4, 4], base=100)
    cc = c.channel()
    cc.basic_qos(prefetch_count=1)
    cc.basic_consume("work", "w2", no_ack=False)
    d = cc.consume_n(1)[0]
    assert d.body == b"work-101"
    cc.basic_nack(d.delivery_tag, requeue=True)
    seen = []
    for _ in range(3):
        d = cc.consume_n(1)[0]
        seen.append((d.body, bool(d.method.redelivered)))
        cc.basic_ack(d.delivery_tag)
    assert seen == [(b"work-101", True), (b"work-102", False), (b"work-100", False)]
    cc.basic_cancel("w2")
    # the ordinary queue beside them is the FIFO it always was
    pc = c.channel()
    pc.basic_consume("plain", "p", no_ack=True)
    assert [d.body for d in pc.consume_n(n)] == [b"plain-%03d" % i for i in range(n)]
    # purge and delete report the count over all priorities
    publish(ch, "byget", [3, 0, 5])
    assert ch.queue_purge("byget") == 3
    assert gc.basic_get("byget", no_ack=True) is None
    publish(ch, "byget", [1, 2])
    assert ch.queue_delete("byget") == 2
    assert (VH, "byget") not in q and len(b.plane.queue_by_slot) == 7
    c.close()


def refusals_script(b):
    """Every 406: a value outside 1 .. 15 or of another type, a different value on a redeclare, the
    argument for an existing ordinary queue, and the argument beside a length limit."""
    from chanamq_amd.client import ChannelClosed, Connection
    c = Connection(port=b.port, vhost="/")

    def refused(name, args, **kw):
        ch = c.channel()
        with pytest.raises(ChannelClosed) as e:
            ch.queue_declare(name, arguments=args, **kw)
        assert e.value.code == 406, (name, args)
        return e.value.text

    for v in BAD_VALUES:
        assert "15" in refused("bad", {"x-max-priority": v})
        assert (VH, "bad") not in b.plane.queues
    ch = c.channel()
    ch.queue_declare("p3", arguments={"x-max-priority": 3})
    ch.queue_declare("plain")
    refused("p3", {"x-max-priority": 4})
    assert "without" in refused("plain", {"x-max-priority": 3})
    if b.queue_limits:
        refused("both", {"x-max-priority": 3, "x-max-length": 10})
        refused("p3", {"x-max-length": 10})
        if b.queue_limit_bytes:
            refused("both", {"x-max-priority": 3, "x-max-length-bytes": 10})
    assert b.plane.queues[(VH, "p3")].max_priority == 3 and b.plane.queues[(VH, "plain")].max_priority is None
    assert len(b.plane.queue_by_slot) == 5
    ch.queue_declare("top", arguments={"x-max-priority": 15})      # the largest served
    assert len(b.plane.queues[(VH, "top")].lanes) == 16
    c.close()


def off_script(b):
    """The option off: the argument is ignored whatever it holds, and the queue is a FIFO."""
    from chanamq_amd.client import Connection
    c = Connection(port=b.port, vhost="/")
    ch = c.channel()
    ch.confirm_select()
    ch.queue_declare("work", arguments={"x-max-priority": 5})
    ch.queue_declare("odd", arguments={"x-max-priority": "many"})
    publish(ch, "work", PRIOS)
    cc = c.channel()
    cc.basic_consume("work", "w", no_ack=True)
    assert [d.body for d in cc.consume_n(len(PRIOS))] == [b"work-%03d" % i for i in range(len(PRIOS))]
    assert all(q.max_priority is None for q in b.plane.queues.values()) and len(b.plane.queue_by_slot) == 2
    assert all("max_priority" not in r for r in rows(b).values())
    c.close()
