"""Conversations with a ``GpuBroker(dead_letter=True)`` about dead-lettering, through the AMQP test
client: shared by tests/test_dlx_broker.py (golden plane, CPU) and tests/test_gpu_dlx_broker.py
(HIP plane).  Every expectation holds however the server cuts the traffic into steps."""

import json
import time

import pytest

from chanamq_amd.protocol.codec import Typed

VH = "AMQ.DEFAULT"
BAD_ARGUMENTS = [{"x-dead-letter-routing-key": "k"}, {"x-dead-letter-exchange": 5},
                 {"x-dead-letter-exchange": Typed("I", 7)}, {"x-dead-letter-exchange": "x" * 256},
                 {"x-dead-letter-exchange": "dlx", "x-dead-letter-routing-key": 1.5},
                 {"x-dead-letter-exchange": "dlx", "x-dead-letter-routing-key": "k" * 256}]
DL_STATS = ("dl_expired", "dl_maxlen", "dl_rejected", "dl_unrouted", "dl_dropped", "dl_pending")


def stats(b, want, seconds=5.0):
    """The broker's /admin/stats fields named in ``want``, once they have reached those values."""
    end = time.time() + seconds
    while True:
        s = json.loads(b.stats_json())
        got = {k: s.get(k) for k in want}
        if got == want or time.time() > end:
            return got
        time.sleep(0.01)


def take(conn, q, n, timeout=10.0):
    cc = conn.channel()
    cc.basic_consume(q, "d-" + q, no_ack=True)
    got = cc.consume_n(n, timeout=timeout)
    cc.basic_cancel("d-" + q)
    return got


def dlx_script(b):
    """A delay queue (expiration + dead-letter exchange) consumed from the parking queue with the
    right exchange and key, with no traffic but the broker's idle steps; reject -> parking queue
    with x-dead-letter-routing-key; a reject on a plain queue stays an ack; the redeclare rule."""
    from chanamq_amd.client import ChannelClosed, Connection
    c = Connection(port=b.port, vhost="/")
    ch = c.channel()
    ch.exchange_declare("dlx", "direct")
    ch.queue_declare("park")
    ch.queue_declare("park.rejected")
    ch.queue_bind("park", "dlx", "delay")
    ch.queue_bind("park.rejected", "dlx", "rejected")
    ch.queue_declare("delay", arguments={"x-dead-letter-exchange": "dlx"})
    ch.queue_declare("work", arguments={"x-dead-letter-exchange": "dlx", "x-dead-letter-routing-key": "rejected"})
    ch.queue_declare("plain")
    q = b.plane.queues
    assert (q[(VH, "delay")].dlx, q[(VH, "delay")].dlk) == ("dlx", None)
    assert (q[(VH, "work")].dlx, q[(VH, "work")].dlk) == ("dlx", b"rejected")
    # the delay queue: nothing consumes it, the messages expire and arrive in the parking queue
    for i in range(3):
        ch.basic_publish("", "delay", b"late-%d" % i, {"expiration": "30", "content_type": "text/plain"})
    got = take(c, "park", 3)
    assert [d.body for d in got] == [b"late-%d" % i for i in range(3)]
    assert all(d.method.exchange == "dlx" and d.method.routing_key == "delay" for d in got)
    assert all(d.props.get("content_type") == "text/plain" for d in got)
    assert stats(b, dict(dl_expired=3, dl_pending=0)) == dict(dl_expired=3, dl_pending=0)
    # reject / nack without requeue -> the parking queue, with the queue's routing key
    for i in range(4):
        ch.basic_publish("", "work", b"job-%d" % i)
    ch.basic_publish("", "plain", b"plain-0")
    w = c.channel()
    w.basic_consume("work", "w", no_ack=False)
    ds = w.consume_n(4)
    w.basic_reject(ds[0].delivery_tag, requeue=False)
    w.basic_ack(ds[1].delivery_tag)
    w.basic_nack(ds[3].delivery_tag, multiple=True, requeue=False)     # 2 and 3
    got = take(c, "park.rejected", 3)
    assert sorted(d.body for d in got) == [b"job-0", b"job-2", b"job-3"]
    assert all(d.method.exchange == "dlx" and d.method.routing_key == "rejected" for d in got)
    p = c.channel()
    p.basic_consume("plain", "p", no_ack=False)
    p.basic_reject(p.consume_n(1)[0].delivery_tag, requeue=False)      # no dead-letter exchange: an ack
    assert stats(b, dict(dl_rejected=3)) == dict(dl_rejected=3)
    assert ch.queue_declare("plain", passive=True).message_count == 0
    assert ch.queue_declare("park.rejected", passive=True).message_count == 0
    # redeclare: the same pair and no pair are no-ops, another pair is 406 with nothing changed
    assert ch.queue_declare("work", arguments={"x-dead-letter-exchange": "dlx",
                                               "x-dead-letter-routing-key": "rejected"}).queue == "work"
    assert ch.queue_declare("work").queue == "work"
    for args in ({"x-dead-letter-exchange": "dlx"}, {"x-dead-letter-exchange": "other", "x-dead-letter-routing-key": "rejected"}):
        bad = c.channel()
        with pytest.raises(ChannelClosed) as e:
            bad.queue_declare("work", arguments=args)
        assert e.value.code == 406
    assert (q[(VH, "work")].dlx, q[(VH, "work")].dlk) == ("dlx", b"rejected")
    c.close()


def refusals_script(b):
    """The key without the exchange, values that are no strings or too long: 406, and no queue."""
    from chanamq_amd.client import ChannelClosed, Connection
    c = Connection(port=b.port, vhost="/")
    for args in BAD_ARGUMENTS:
        ch = c.channel()
        with pytest.raises(ChannelClosed) as e:
            ch.queue_declare("bad", arguments=args)
        assert e.value.code == 406, args
        assert (VH, "bad") not in b.plane.queues
    ch = c.channel()
    ch.queue_declare("bad", arguments={"x-dead-letter-exchange": "not-yet-declared"})   # it need not exist
    assert b.plane.queues[(VH, "bad")].dlx == "not-yet-declared"
    c.close()


def off_script(b):
    """The option off: the arguments are ignored (invalid ones too), an expired message is gone."""
    from chanamq_amd.client import Connection
    c = Connection(port=b.port, vhost="/")
    ch = c.channel()
    ch.exchange_declare("dlx", "fanout")
    ch.queue_declare("park")
    ch.queue_bind("park", "dlx", "")
    ch.queue_declare("delay", arguments={"x-dead-letter-exchange": "dlx"})
    ch.queue_declare("odd", arguments={"x-dead-letter-routing-key": 5})
    ch.basic_publish("", "delay", b"gone", {"expiration": "10"})
    ch.basic_publish("", "delay", b"stays")
    time.sleep(0.1)
    assert [d.body for d in take(c, "delay", 1)] == [b"stays"]
    assert ch.queue_declare("park", passive=True).message_count == 0
    s = json.loads(b.stats_json())
    assert not any(k in s for k in DL_STATS)
    assert getattr(b.plane.queues[(VH, "delay")], "dlx", None) is None
    c.close()
