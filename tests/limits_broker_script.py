"""Conversations with a ``GpuBroker(queue_limits=True)`` about queue length limits, through the
AMQP test client: shared by tests/test_limits_broker.py (golden plane, CPU) and
tests/test_gpu_limits_broker.py (HIP plane).  Every expectation holds however the server cuts
the publishes into steps: a drop-head queue without a consumer keeps the newest L at the end of
every step, a reject-publish queue without one keeps the first L."""

import json
import time

import pytest

from chanamq_amd.protocol.codec import Typed

VH = "AMQ.DEFAULT"
N = 10
BAD_ARGUMENTS = [{"x-max-length": -1}, {"x-max-length": "10"}, {"x-max-length": 1.5}, {"x-max-length": True},
                 {"x-max-length": 3, "x-overflow": "reject-publish-dlx"}, {"x-overflow": "drop-tail"},
                 {"x-max-length": 3, "x-overflow": 1}]


def bodies(lo, hi, tag=""):
    return [f"{tag}{i}".encode() for i in range(lo, hi)]


def stats(b, want, seconds=5.0):
    """The broker's /admin/stats fields named in ``want``, once they have reached those values
    (the pipelined front end hands its counters over with its next event)."""
    end = time.time() + seconds
    while True:
        s = json.loads(b.stats_json())
        got = {k: s.get(k) for k in want}
        if got == want or time.time() > end:
            return got
        time.sleep(0.01)


def publish_confirmed(ch, q, lo, hi, tag=""):
    for body in bodies(lo, hi, tag):
        ch.basic_publish("", q, body)
    return ch.wait_for_confirms()


def drain(conn, q, n):
    cc = conn.channel()
    cc.basic_consume(q, "d-" + q, no_ack=True)
    got = [d.body for d in cc.consume_n(n)]
    cc.basic_cancel("d-" + q)
    return got


def limits_script(b):
    """Declare with arguments, both modes; redeclare with an equal limit and with a different
    one; both counters in the stats."""
    from chanamq_amd.client import ChannelClosed, Connection
    c = Connection(port=b.port, vhost="/")
    ch = c.channel()
    ch.confirm_select()
    ch.queue_declare("keep2", arguments={"x-max-length": 2, "x-max-length-bytes": 1})        # (bytes: ignored)
    ch.queue_declare("first3", arguments={"x-max-length": Typed("l", 3), "x-overflow": "reject-publish"})
    ch.queue_declare("nothing", arguments={"x-max-length": 0, "x-overflow": "drop-head"})
    q = b.plane.queues
    assert [(q[(VH, n)].max_length, q[(VH, n)].overflow) for n in ("keep2", "first3", "nothing")] == [
        (2, "drop-head"), (3, "reject-publish"), (0, "drop-head")]
    assert publish_confirmed(ch, "keep2", 0, N) is True               # trimmed, never nacked
    assert publish_confirmed(ch, "first3", 0, N) is False             # 7 refused: Basic.Nack
    assert publish_confirmed(ch, "nothing", 0, N) is True
    assert [ch.queue_declare(n, passive=True).message_count for n in ("keep2", "first3", "nothing")] == [2, 3, 0]
    assert stats(b, dict(maxlen_dropped=N - 2 + N, maxlen_rejected=N - 3)) == dict(maxlen_dropped=2 * N - 2,
                                                                                  maxlen_rejected=N - 3)
    assert drain(c, "keep2", 2) == bodies(N - 2, N) and drain(c, "first3", 3) == bodies(0, 3)
    assert publish_confirmed(ch, "first3", N, N + 2) is True          # drained: it takes publishes again
    assert drain(c, "first3", 2) == bodies(N, N + 2)
    # a redeclare with the same limit is the usual no-op, one without arguments too
    assert ch.queue_declare("keep2", arguments={"x-max-length": 2}).message_count == 0
    assert ch.queue_declare("keep2").queue == "keep2"
    assert ch.queue_declare("first3", arguments={"x-max-length": 3, "x-overflow": "reject-publish"}).queue == "first3"
    for name, args in (("keep2", {"x-max-length": 3}), ("keep2", {"x-max-length": 2, "x-overflow": "reject-publish"}),
                       ("first3", {"x-max-length": 3})):
        bad = c.channel()
        with pytest.raises(ChannelClosed) as e:
            bad.queue_declare(name, arguments=args)
        assert e.value.code == 406
    assert (q[(VH, "keep2")].max_length, q[(VH, "keep2")].overflow) == (2, "drop-head")
    assert (q[(VH, "first3")].max_length, q[(VH, "first3")].overflow) == (3, "reject-publish")
    c.close()


def refusals_script(b):
    """A length that is no integer >= 0, or an unknown mode: 406, and no queue."""
    from chanamq_amd.client import ChannelClosed, Connection
    c = Connection(port=b.port, vhost="/")
    for args in BAD_ARGUMENTS:
        ch = c.channel()
        with pytest.raises(ChannelClosed) as e:
            ch.queue_declare("bad", arguments=args)
        assert e.value.code == 406, args
        assert (VH, "bad") not in b.plane.queues
    ch = c.channel()
    ch.queue_declare("bad", arguments={"x-max-length": 1})            # the name is still free, and works
    assert b.plane.queues[(VH, "bad")].max_length == 1
    c.close()


def off_script(b):
    """The option off: 10 messages into an x-max-length = 2 queue all arrive, invalid values pass."""
    from chanamq_amd.client import Connection
    c = Connection(port=b.port, vhost="/")
    ch = c.channel()
    ch.confirm_select()
    ch.queue_declare("keep2", arguments={"x-max-length": 2})
    ch.queue_declare("first3", arguments={"x-max-length": 3, "x-overflow": "reject-publish"})
    ch.queue_declare("odd", arguments={"x-max-length": -5, "x-overflow": "whatever"})
    assert publish_confirmed(ch, "keep2", 0, N) is True and publish_confirmed(ch, "first3", 0, N) is True
    assert drain(c, "keep2", N) == bodies(0, N) and drain(c, "first3", N) == bodies(0, N)
    s = json.loads(b.stats_json())
    assert "maxlen_dropped" not in s and "maxlen_rejected" not in s
    assert getattr(b.plane.queues[(VH, "keep2")], "max_length", None) is None
    c.close()


def durable_before(port):
    """A durable queue with a limit, 6 persistent messages: the newest 4 are stored."""
    from chanamq_amd.client import Connection
    c = Connection(port=port, vhost="/")
    ch = c.channel()
    ch.confirm_select()
    ch.queue_declare("dur.lim", durable=True, arguments={"x-max-length": 4})
    for body in bodies(0, 6, "one:"):
        ch.basic_publish("", "dur.lim", body, {"delivery_mode": 2})
    assert ch.wait_for_confirms() is True
    assert ch.queue_declare("dur.lim", durable=True, passive=True).message_count == 4
    c.close()


def durable_after(b):
    """After the restart the queue is back with its 4 messages and without a limit (the store
    keeps none): it takes 3 more.  The first declare that carries a limit is adopted, the queue
    trims to it at its next step, and the next declare must agree."""
    from chanamq_amd.client import ChannelClosed, Connection
    q = b.plane.queues[(VH, "dur.lim")]
    assert q.max_length is None
    c = Connection(port=b.port, vhost="/")
    ch = c.channel()
    ch.confirm_select()
    assert ch.queue_declare("dur.lim", durable=True, passive=True).message_count == 4
    for body in bodies(0, 3, "two:"):
        ch.basic_publish("", "dur.lim", body, {"delivery_mode": 2})
    assert ch.wait_for_confirms() is True
    assert ch.queue_declare("dur.lim", durable=True).message_count == 7
    ch.queue_declare("dur.lim", durable=True, arguments={"x-max-length": 2})
    assert (q.max_length, q.overflow) == (2, "drop-head")
    ch.basic_publish("", "dur.lim", b"three:0", {"delivery_mode": 2})
    assert ch.wait_for_confirms() is True
    assert ch.queue_declare("dur.lim", durable=True, passive=True).message_count == 2
    bad = c.channel()
    with pytest.raises(ChannelClosed) as e:
        bad.queue_declare("dur.lim", durable=True, arguments={"x-max-length": 4})
    assert e.value.code == 406
    assert drain(c, "dur.lim", 2) == [b"two:2", b"three:0"]
    c.close()
