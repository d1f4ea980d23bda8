"""Headers exchanges through the server: ``GpuBroker(headers_match=True)`` on the golden plane
(CPU), spoken to by the AMQP test client.  tests/test_gpu_headers_broker.py runs the same
conversations on the HIP plane."""

import pytest

from headers_broker_script import (DURABLE_EXPECTED, EXPECTED, EXPECTED_OFF, MESSAGES, QUEUES, UNBIND_EXPECTED, collect,
                                   durable_check, durable_setup, publish_all, script, unbind_script)

SMALL = dict(c_max=64, chpc=8, q_max=64, x_max=64, cons_max=256, ucap=256, deliver_cap=4096)


def golden(on=True, **kw):
    from chanamq_amd.engine.golden import GoldenDataPlane
    g = GoldenDataPlane(default_queue_capacity=1 << 12, ring_pool=1 << 20, **dict(SMALL, **kw),
                        **({"headers_match": True} if on else {}))
    g.hb_max, g.hp_max = 8, 12
    return g


def serve(plane, io="python", **kw):
    from chanamq_amd.server.gpu_broker import GpuBroker
    return GpuBroker(plane, idle_step_ms=1.0, io=io, ingress_bytes=8 << 20, **kw).start()


def refusals(b):
    """Each bound refused with 506 (a connection exception, as for the exchange-to-exchange
    bounds): nothing changed, and the bindings made before and after keep working."""
    from chanamq_amd.client import Connection, ConnectionClosed
    from chanamq_amd import ops
    pairs = int(ops.load().HB_PAIRS)

    def refused(*args):
        bad = Connection(port=b.port, vhost="/")
        before = sorted(map(repr, b.plane.exchanges[("AMQ.DEFAULT", "hr")].hbindings))
        with pytest.raises(ConnectionClosed) as e:
            bad.channel().queue_bind(*args)
        assert e.value.code == 506
        assert sorted(map(repr, b.plane.exchanges[("AMQ.DEFAULT", "hr")].hbindings)) == before
    c = Connection(port=b.port, vhost="/")
    ch = c.channel()
    ch.exchange_declare("hr", "headers")
    ch.queue_declare("r")
    ch.queue_bind("r", "hr", "", {"keep": "1"})
    refused("r", "hr", "", {f"p{i}": "v" for i in range(pairs + 1)})
    ch.queue_bind("r", "hr", "", {f"p{i}": "v" for i in range(b.plane.hp_max - 1)})     # the pool's last pair
    refused("r", "hr", "", {"one": "more"})
    for i in range(b.plane.hb_max - 2):
        ch.queue_bind("r", "hr", f"k{i}", {"x-match": "any"} if i else {"x-match": "all", "x-note": "no pairs"})
    refused("r", "hr", "past", {})                                                    # one past the table's last row
    ch.queue_unbind("r", "hr", "k0", {})
    cc = c.channel()
    cc.basic_consume("r", "r", no_ack=True)
    ch.basic_publish("hr", "", b"kept", {"headers": {"keep": "1"}})
    assert [d.body for d in cc.consume_n(1)] == [b"kept"]
    c.close()


def conversations(b):
    assert script(b.port) == EXPECTED
    assert unbind_script(b.port) == UNBIND_EXPECTED


@pytest.mark.parametrize("io", ["native", "python"])
def test_server_on_golden_plane(io):
    b = serve(golden(), io, headers_match=True)
    try:
        conversations(b)
    finally:
        b.stop()


def test_refusals_leave_the_other_bindings_working():
    b = serve(golden(), headers_match=True)
    try:
        refusals(b)
    finally:
        b.stop()


def test_exchange_bind_arguments_reach_the_plane():
    """Both options on: an edge out of a headers source is matched on its arguments."""
    from chanamq_amd.client import Connection
    b = serve(golden(), headers_match=True, exchange_bindings=True)
    try:
        c = Connection(port=b.port, vhost="/")
        ch = c.channel()
        ch.exchange_declare("src", "headers")
        ch.exchange_declare("dst", "fanout")
        ch.queue_declare("behind")
        ch.queue_bind("behind", "dst", "")
        ch.exchange_bind("dst", "src", "", {"go": "yes"})
        ch.exchange_bind("dst", "src", "", {"go": "yes"})
        cc = c.channel()
        cc.basic_consume("behind", "behind", no_ack=True)
        for body, h in ((b"1", {"go": "yes"}), (b"2", {"go": "no"}), (b"3", {"go": "yes", "x": 1})):
            ch.basic_publish("src", "", body, {"headers": h})
        assert [d.body for d in cc.consume_n(2)] == [b"1", b"3"]
        ch.exchange_unbind("dst", "src", "", {"go": "no"})
        ch.basic_publish("src", "", b"4", {"headers": {"go": "yes"}})
        assert [d.body for d in cc.consume_n(1)] == [b"4"]
        ch.exchange_unbind("dst", "src", "", {"go": "yes"})
        ch.basic_publish("src", "", b"5", {"headers": {"go": "yes"}})
        ch.queue_bind("behind", "src", "", {"last": None})
        ch.basic_publish("src", "", b"6", {"headers": {"last": 0}})
        assert [d.body for d in cc.consume_n(1)] == [b"6"]
        c.close()
    finally:
        b.stop()


def test_option_off_answers_and_routes_as_before():
    """Off (the default): arguments are dropped, a headers exchange routes as topic, and the
    plane keeps no argument bindings."""
    from chanamq_amd.client import Connection
    b = serve(golden(on=False))
    try:
        assert b.headers_match is False
        c = Connection(port=b.port, vhost="/")
        ch = c.channel()
        ch.exchange_declare("hx", "headers")
        from headers_broker_script import BINDS
        for q in QUEUES:
            ch.queue_declare(q)
            ch.queue_bind(q, "hx", "", BINDS[q])
        cc = c.channel()
        for q in QUEUES:
            cc.basic_consume(q, q, no_ack=True)
        publish_all(ch, "hx")
        assert collect(cc, len(QUEUES) * len(MESSAGES)) == EXPECTED_OFF
        ch.queue_unbind("q_all", "hx", "", {"other": "arguments"})      # arguments play no part: it goes
        ch.basic_publish("hx", "", b"after", {"headers": {"region": "eu", "tier": "gold"}})
        assert sorted(collect(cc, len(QUEUES) - 1)) == sorted(set(QUEUES) - {"q_all"})
        c.close()
        x = b.plane.exchanges[("AMQ.DEFAULT", "hx")]
        assert not x.hbindings and len(x.bindings) == len(QUEUES) - 1
    finally:
        b.stop()
    with pytest.raises(ValueError):
        serve(golden(on=False), headers_match=True)


def test_config_keys_reach_plane_and_broker(tmp_path):
    from chanamq_amd.utils.config import Config
    plane, broker = Config.load([], {}).gpu_config()
    assert broker["headers_match"] is False and "headers_match" not in plane and "hb_max" not in plane
    f = tmp_path / "on.conf"
    f.write_text("chana.mq.gpu.headers-match = true\nchana.mq.gpu.headers-bindings = 77\n")
    for single in (True, False):
        plane, broker = Config.load([str(f)], {}).gpu_config(single=single)
        assert broker["headers_match"] is True and plane["headers_match"] is True and plane["hb_max"] == 77


def test_control_log_carries_the_arguments():
    """The replicated ops carry canonical arguments as JSON and give them back unchanged."""
    import json
    from decimal import Decimal
    from chanamq_amd.models.matcher import args_from_map, args_json, args_to_map, args_unjson, canon_args
    from chanamq_amd.parallel.control_log import ControlLog
    from chanamq_amd.protocol.codec import Typed
    args = {"x-match": "any", "v": None, "i": Typed("l", -7), "f": 2.5, "D": Decimal("1.50"), "t": [1, {"k": b"\xff"}],
            "s": "text", "n\xe9": b"\x00\xff"}
    want = canon_args(args)
    assert args_unjson(json.loads(json.dumps(args_json(args)))) == want
    assert args_from_map(args_to_map([want, canon_args({})])) == [want, canon_args({})]
    assert args_from_map({}) == [canon_args(None)]

    class Plane:
        def bind(self, *a):
            self.got = a
        unbind = bind
    p = Plane()
    log = ControlLog(p, comm=None)
    log.submit("bind", "vh", "q", "x", "k", args)
    op, a, kw = json.loads(json.dumps(log.outbox[0]))
    log._apply(op, a, kw)
    assert p.got[:4] == ("vh", "q", "x", "k") and p.got[4] == want
    log.submit("unbind", "vh", "q", "x", "k")
    log.submit("bind", "vh", "q", "x", "k", None)
    for op, a, kw in log.outbox[1:]:
        log._apply(op, a, kw)
        assert p.got[4:] in ((), (None,))


def test_durable_bindings_survive_a_restart_with_their_arguments(tmp_path):
    from chanamq_amd.broker import load
    core = load()

    def boot():
        st = core.Store()
        st.open(str(tmp_path / "store"), True)
        return st, serve(golden(persist=True), "python", store=st, headers_match=True)
    st, b = boot()
    try:
        durable_setup(b.port)
        assert durable_check(b.port, "one") == sorted("one:" + m for m in DURABLE_EXPECTED)
        before = sorted(map(repr, b.plane.exchanges[("AMQ.DEFAULT", "dur.h")].hbindings))
    finally:
        b.stop()
        st.close()
    st, b = boot()
    try:
        assert sorted(map(repr, b.plane.exchanges[("AMQ.DEFAULT", "dur.h")].hbindings)) == before and len(before) == 3
        assert durable_check(b.port, "two") == sorted("two:" + m for m in DURABLE_EXPECTED)
        # an unbind of one of the three reaches the store: after another restart two are left
        from chanamq_amd.client import Connection
        c = Connection(port=b.port, vhost="/")
        c.channel().queue_unbind("dur.q", "dur.h", "k", {"d": 2.5})
        c.close()
    finally:
        b.stop()
        st.close()
    st, b = boot()
    try:
        assert len(b.plane.exchanges[("AMQ.DEFAULT", "dur.h")].hbindings) == 2
    finally:
        b.stop()
        st.close()
