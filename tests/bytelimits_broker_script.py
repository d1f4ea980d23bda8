"""Conversations with a ``GpuBroker(queue_limits=True, queue_limit_bytes=True)`` about queue byte
limits, through the AMQP test client: shared by tests/test_bytelimits_broker.py (golden plane,
CPU) and tests/test_gpu_bytelimits_broker.py (HIP plane).  Every body is 10 bytes, and every
expectation holds however the server cuts the publishes into steps: a drop-head queue without a
consumer holds at most B bytes at the end of every step (the newest), a reject-publish queue
without one takes publishes until its ready bytes reach B (the first)."""

import json

import pytest

from chanamq_amd.protocol.codec import Typed
from limits_broker_script import drain, stats

VH = "AMQ.DEFAULT"
N = 10
WIDE = (1 << 32) + 5
BAD_ARGUMENTS = [{"x-max-length-bytes": -1}, {"x-max-length-bytes": "10"}, {"x-max-length-bytes": 1.5},
                 {"x-max-length-bytes": True}, {"x-max-length-bytes": 3, "x-overflow": "drop-tail"},
                 {"x-max-length-bytes": 3, "x-overflow": 1}, {"x-max-length": 3, "x-max-length-bytes": -2}]


def bodies(lo, hi):
    return [b"%010d" % i for i in range(lo, hi)]


def publish_confirmed(ch, q, lo, hi):
    for body in bodies(lo, hi):
        ch.basic_publish("", q, body)
    return ch.wait_for_confirms()


def rows(b):
    return {r["name"]: r for r in json.loads(b.queues_json())}


def bytelimits_script(b):
    """Declare with the argument in both modes, alone and beside x-max-length, in 64 bits; what a
    confirming publisher and a consumer see; ready_bytes in the admin rows; redeclares."""
    from chanamq_amd.client import ChannelClosed, Connection
    c = Connection(port=b.port, vhost="/")
    ch = c.channel()
    ch.confirm_select()
    ch.queue_declare("keep20", arguments={"x-max-length-bytes": 20})
    ch.queue_declare("first25", arguments={"x-max-length-bytes": Typed("l", 25), "x-overflow": "reject-publish"})
    ch.queue_declare("both", arguments={"x-max-length": 5, "x-max-length-bytes": Typed("s", 30)})
    ch.queue_declare("wide", arguments={"x-max-length-bytes": Typed("l", WIDE), "x-overflow": "reject-publish"})
    ch.queue_declare("plain")
    q = b.plane.queues
    assert [(q[(VH, n)].max_length, q[(VH, n)].max_length_bytes, q[(VH, n)].overflow)
            for n in ("keep20", "first25", "both", "wide", "plain")] == [
        (None, 20, "drop-head"), (None, 25, "reject-publish"), (5, 30, "drop-head"), (None, WIDE, "reject-publish"),
        (None, None, "drop-head")]
    assert publish_confirmed(ch, "keep20", 0, N) is True               # trimmed, never nacked
    assert publish_confirmed(ch, "first25", 0, N) is False             # 0, 10, 20 < 25: three taken, 7 refused
    assert publish_confirmed(ch, "both", 0, N) is True
    assert publish_confirmed(ch, "wide", 0, N) is True                 # 2^32 + 5 is not 5
    assert publish_confirmed(ch, "plain", 0, N) is True
    names = ("keep20", "first25", "both", "wide", "plain")
    assert [ch.queue_declare(n, passive=True).message_count for n in names] == [2, 3, 3, N, N]
    want = dict(maxlen_dropped=(N - 2) + (N - 3), maxlen_rejected=N - 3)
    assert stats(b, want) == want
    r = rows(b)
    assert [(r[n]["ready"], r[n]["ready_bytes"]) for n in names] == [(2, 20), (3, 30), (3, 30), (N, 10 * N), (N, 10 * N)]
    assert drain(c, "keep20", 2) == bodies(N - 2, N) and drain(c, "first25", 3) == bodies(0, 3)
    assert drain(c, "both", 3) == bodies(N - 3, N) and drain(c, "wide", N) == bodies(0, N)
    assert publish_confirmed(ch, "first25", N, N + 2) is True          # drained: it takes publishes again
    assert drain(c, "first25", 2) == bodies(N, N + 2)
    r = rows(b)
    assert [(r[n]["ready"], r[n]["ready_bytes"]) for n in names] == [(0, 0)] * 4 + [(N, 10 * N)]
    # a redeclare with the same value is the usual no-op, one without the argument too
    assert ch.queue_declare("keep20", arguments={"x-max-length-bytes": 20}).message_count == 0
    assert ch.queue_declare("keep20").queue == "keep20"
    assert ch.queue_declare("first25", arguments={"x-max-length-bytes": 25, "x-overflow": "reject-publish"}).queue == "first25"
    for name, args in (("keep20", {"x-max-length-bytes": 21}), ("keep20", {"x-max-length-bytes": 20, "x-overflow": "reject-publish"}),
                       ("first25", {"x-max-length-bytes": 25}), ("wide", {"x-max-length-bytes": 5, "x-overflow": "reject-publish"}),
                       ("both", {"x-max-length": 5, "x-max-length-bytes": 31})):
        bad = c.channel()
        with pytest.raises(ChannelClosed) as e:
            bad.queue_declare(name, arguments=args)
        assert e.value.code == 406, (name, args)
    assert (q[(VH, "keep20")].max_length_bytes, q[(VH, "keep20")].overflow) == (20, "drop-head")
    assert (q[(VH, "both")].max_length, q[(VH, "both")].max_length_bytes) == (5, 30)
    assert q[(VH, "wide")].max_length_bytes == WIDE
    c.close()


def refusals_script(b):
    """A value that is no integer >= 0, or an unknown mode: 406, and no queue."""
    from chanamq_amd.client import ChannelClosed, Connection
    c = Connection(port=b.port, vhost="/")
    for args in BAD_ARGUMENTS:
        ch = c.channel()
        with pytest.raises(ChannelClosed) as e:
            ch.queue_declare("bad", arguments=args)
        assert e.value.code == 406, args
        assert (VH, "bad") not in b.plane.queues
    ch = c.channel()
    ch.queue_declare("bad", arguments={"x-max-length-bytes": 0})       # the name is still free; B = 0 is legal
    assert b.plane.queues[(VH, "bad")].max_length_bytes == 0
    c.close()


def off_script(b):
    """``queue-limits`` on, ``queue-limit-bytes`` off: the argument is ignored whatever it holds,
    the count limit beside it still works, and the admin rows carry no ready_bytes."""
    from chanamq_amd.client import Connection
    c = Connection(port=b.port, vhost="/")
    ch = c.channel()
    ch.confirm_select()
    ch.queue_declare("keep20", arguments={"x-max-length-bytes": 20})
    ch.queue_declare("first25", arguments={"x-max-length-bytes": 25, "x-overflow": "reject-publish"})
    ch.queue_declare("odd", arguments={"x-max-length-bytes": -5})
    ch.queue_declare("keep2", arguments={"x-max-length": 2, "x-max-length-bytes": 1})
    assert publish_confirmed(ch, "keep20", 0, N) is True and publish_confirmed(ch, "first25", 0, N) is True
    assert publish_confirmed(ch, "keep2", 0, N) is True
    assert drain(c, "keep20", N) == bodies(0, N) and drain(c, "first25", N) == bodies(0, N)
    assert drain(c, "keep2", 2) == bodies(N - 2, N)
    assert all("ready_bytes" not in r for r in rows(b).values())
    assert all(getattr(q, "max_length_bytes", None) is None for q in b.plane.queues.values())
    c.close()
