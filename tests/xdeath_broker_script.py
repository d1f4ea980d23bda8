"""Conversations with a ``GpuBroker(dead_letter=True, x_death=True)`` through the AMQP test client:
shared by tests/test_xdeath_broker.py (golden plane, CPU) and tests/test_gpu_xdeath_broker.py (HIP
plane).  Every expectation holds however the server cuts the traffic into steps."""

import time

from chanamq_amd.protocol.codec import Typed
from dlx_broker_script import stats, take


def xdeath_script(b):
    """A message with a TTL in a queue with a dead-letter exchange reaches the parking queue's
    consumer with the x-death entry a client expects; a retry by reject through the same queue
    counts up; a queue that dead-letters into itself by TTL ends empty, with dl_cycle counted."""
    from chanamq_amd.client import Connection
    c = Connection(port=b.port, vhost="/")
    ch = c.channel()
    ch.exchange_declare("dlx", "direct")
    ch.queue_declare("park")
    ch.queue_bind("park", "dlx", "delay")
    ch.queue_declare("delay", arguments={"x-dead-letter-exchange": "dlx"})
    t0 = int(time.time())
    ch.basic_publish("", "delay", b"late", {"expiration": "30", "content_type": "text/plain", "headers": {"job": 7}})
    d = take(c, "park", 1)[0]
    t1 = int(time.time())
    assert d.body == b"late" and d.method.exchange == "dlx" and d.method.routing_key == "delay"
    assert d.props.get("content_type") == "text/plain" and d.props.get("expiration") is None
    h = d.props["headers"]
    assert list(h) == ["job", "x-first-death-reason", "x-first-death-queue", "x-first-death-exchange", "x-death"]
    assert (h["job"], h["x-first-death-reason"], h["x-first-death-queue"], h["x-first-death-exchange"]) == (7, "expired", "delay", "")
    assert len(h["x-death"]) == 1
    x = dict(h["x-death"][0])
    t = x.pop("time")
    assert isinstance(t, Typed) and t.tag == "T" and t0 - 1 <= t.value <= t1 + 1
    assert x == {"count": Typed("l", 1), "reason": "expired", "queue": "delay", "exchange": "",
                 "routing-keys": ["delay"], "original-expiration": "30"}
    # retry with back-off as clients build it: reject -> the same queue again, x-death[0].count goes up
    ch.exchange_declare("retry", "fanout")
    ch.queue_declare("work", arguments={"x-dead-letter-exchange": "retry"})
    ch.queue_bind("work", "retry", "")
    ch.basic_publish("", "work", b"job")
    w = c.channel()
    w.basic_consume("work", "w", no_ack=False)
    for n in (None, 1, 2):
        dv = w.consume_n(1)[0]
        xd = (dv.props.get("headers") or {}).get("x-death")
        assert (None if xd is None else xd[0]["count"].value) == n and (xd is None or len(xd) == 1)
        if n == 2:
            w.basic_ack(dv.delivery_tag)
        else:
            w.basic_reject(dv.delivery_tag, requeue=False)
    # a queue that dead-letters into itself by TTL: refused, the queue ends empty
    ch.exchange_declare("loop", "fanout")
    ch.queue_declare("self", arguments={"x-dead-letter-exchange": "loop", "x-message-ttl": 20})
    ch.queue_bind("self", "loop", "")
    ch.basic_publish("", "self", b"round")
    assert stats(b, dict(dl_cycle=1, dl_pending=0)) == dict(dl_cycle=1, dl_pending=0)
    assert ch.queue_declare("self", passive=True).message_count == 0
    c.close()
