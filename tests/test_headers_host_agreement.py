"""The two front ends of the project agree on what a headers exchange does: the traffic of the
``modes``, the string / integer / boolean part of ``value_types`` and ``entry_chunks``
scenarios, and the server conversation, through the native host broker (``_core``,
csrc/core/broker.cpp headers_match) yield the message sets the scenarios' brute-force matcher
works out -- the same sets the golden model and the HIP plane are held to.

Excluded, as the documented difference (CHANGES.md "Headers exchanges"): the raw class.  The
host renders a float or double as text (so the double 1.5 equals the string "1.5" there), a
decimal as its unscaled integer and arrays and tables as the integer 0; the GPU path compares
such values by tag and wire bytes only."""

import pytest

from gpu_cfg import CFG
from headers_broker_script import EXPECTED, script
from headers_scenarios import HWorld, golden_plane, limits, sc_entry_chunks, sc_modes, sc_value_types

RAW_CLASS_EXCLUDED = "f d D A F"      # see the module docstring


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    from chanamq_amd.broker import load
    hb = load().Broker({"port": 0, "host": "127.0.0.1", "heartbeat": 0,
                        "data_dir": str(tmp_path_factory.mktemp("host") / "data")})
    hb.start()
    yield hb
    hb.stop()


def test_server_conversation(host):
    """The same conversation with both front ends: the native host broker and
    ``GpuBroker(headers_match=True)`` on the golden plane answer with the same message sets.
    (Not the unbind conversation: the host keeps one binding per queue and key, whatever its
    arguments -- a documented difference.)"""
    from test_headers_broker import golden, serve
    b = serve(golden(), headers_match=True)
    try:
        assert script(b.port) == script(host.port) == EXPECTED
    finally:
        b.stop()


SCENARIOS = {"modes": sc_modes, "value_types": lambda dp, lim: sc_value_types(dp, lim, raw=False),
             "entry_chunks": sc_entry_chunks}


@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_scenario_traffic_yields_the_same_sets(host, name, monkeypatch):
    from chanamq_amd.client import Connection
    calls = []
    real_bind, real_pub = HWorld.hbind, HWorld.hpub

    def hbind(self, q, x, args, key=""):
        calls.append(("bind", q, x, dict(args), key))
        return real_bind(self, q, x, args, key)

    def hpub(self, conn, x, headers=None, key="", **kw):
        data = real_pub(self, conn, x, headers, key, **kw)
        h = list(headers.items()) if isinstance(headers, dict) else headers
        calls.append(("pub", x, h, key, self.pubs[-1].body, list(self.pubs[-1].queues)))
        return data
    monkeypatch.setattr(HWorld, "hbind", hbind)
    monkeypatch.setattr(HWorld, "hpub", hpub)
    # a golden plane stands where a scenario expects one while it is built: HWorld records the
    # topology and the traffic, which are then replayed against the host broker
    run = SCENARIOS[name](golden_plane(dict(CFG, q_max=128, hb_max=256, hp_max=1024)), limits())
    assert run.pubs
    pre = f"{name}."
    c = Connection(port=host.port, vhost="/")
    ch = c.channel()
    queues, want = [], {}
    for call in calls:
        if call[0] == "bind":
            _, q, x, args, key = call
            ch.exchange_declare(pre + x, "headers")
            if q not in queues:
                queues.append(q)
                ch.queue_declare(pre + q, exclusive=True)
            ch.queue_bind(pre + q, pre + x, key, args)
    cc = c.channel()
    for q in queues:
        cc.basic_consume(pre + q, q, no_ack=True)
    n = 0
    for call in calls:
        if call[0] == "pub":
            _, x, h, key, body, qs = call
            if h is not None and len({k for k, _ in h}) != len(h):
                continue        # (the client's table is a dict: duplicate names cannot be sent through it)
            ch.basic_publish(pre + x, key, body, {} if h is None else {"headers": dict(h)})
            for q in qs:
                want.setdefault(q, []).append(body)
                n += 1
    got = {}
    for d in cc.consume_n(n):
        got.setdefault(d.method.consumer_tag, []).append(d.body)
    # nothing more arrives: a publish every queue of the scenario takes closes the stream
    ch.exchange_declare(pre + "end", "fanout")
    for q in queues:
        ch.queue_bind(pre + q, pre + "end", "")
    ch.basic_publish(pre + "end", "", b"end")
    tail = [d.body for d in cc.consume_n(len(queues))]
    assert tail == [b"end"] * len(queues)
    assert got == want
    c.close()
