"""The alternate-exchange conversation with a ``GpuBroker(alternate_exchange=True)`` through the
AMQP test client: shared by tests/test_alt_broker.py (golden plane, CPU) and
tests/test_gpu_alt_broker.py (HIP plane).  Every expectation holds however the server cuts the
traffic into steps."""

import pytest

from dlx_broker_script import stats, take

ALT = "alternate-exchange"


def alt_script(b):
    """Declare with the argument; a mandatory publish to a missing key arrives on the catch-all
    queue with no Basic.Return; with the alternate deleted the same publish comes back with 312; a
    redeclare that names another alternate closes the channel with 406; alt_routed counts."""
    from chanamq_amd.client import ChannelClosed, Connection
    c = Connection(port=b.port, vhost="/")
    ch = c.channel()
    ch.exchange_declare("ae", "fanout")
    ch.exchange_declare("front", "direct", arguments={ALT: "ae"})
    ch.queue_declare("catchall")
    ch.queue_bind("catchall", "ae", "")
    ch.queue_declare("known")
    ch.queue_bind("known", "front", "known")
    ch.confirm_select()
    # (a return precedes the publish's confirm: once the confirm is here, so is any return)
    ch.basic_publish("front", "missing", b"caught", mandatory=True)
    ch.basic_publish("front", "known", b"routed", mandatory=True)
    assert ch.wait_for_confirms() and not ch.returns
    d = take(c, "catchall", 1)[0]
    assert (d.body, d.method.exchange, d.method.routing_key) == (b"caught", "front", "missing")
    assert take(c, "known", 1)[0].body == b"routed"
    assert stats(b, dict(alt_routed=1)) == dict(alt_routed=1)
    ch.exchange_declare("front", "direct")                            # no argument: the no-op
    ch.exchange_declare("front", "direct", arguments={ALT: "ae"})     # the same: fine
    ch.exchange_delete("ae")
    ch.basic_publish("front", "missing", b"dropped", mandatory=True)
    assert ch.wait_for_confirms()
    assert [(r.method.reply_code, r.body) for r in ch.returns] == [(312, b"dropped")]
    assert ch.queue_declare("catchall", passive=True).message_count == 0
    assert stats(b, dict(alt_routed=1)) == dict(alt_routed=1)
    for bad in ({ALT: "other"}, {ALT: 5}):
        ch2 = c.channel()
        with pytest.raises(ChannelClosed) as e:
            ch2.exchange_declare("front", "direct", arguments=bad)
        assert e.value.code == 406, bad
    c.close()
