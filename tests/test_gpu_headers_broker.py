"""Headers exchanges through the server on the HIP data plane: the conversations of
tests/headers_broker_script.py against ``GpuBroker(headers_match=True)`` over a
``GpuDataPlane(headers_match=True)``, with the Python-stepped and the pipelined front end."""

import pytest

from gpu_cfg import CFG
from headers_broker_script import (BINDS, DURABLE_EXPECTED, EXPECTED_OFF, MESSAGES, QUEUES, collect, durable_check,
                                   durable_setup, publish_all)
from test_headers_broker import conversations, refusals, serve

pytestmark = pytest.mark.gpu


def plane(on=True, **kw):
    from chanamq_amd.engine.dataplane import GpuDataPlane
    cfg = dict(CFG, default_queue_capacity=1 << 12, **kw)
    if on:
        cfg.update(headers_match=True, hb_max=8, hp_max=12)
    return GpuDataPlane(**cfg)


@pytest.mark.parametrize("io", ["native", "pipeline"])
def test_server_on_gpu_plane(gpu, io):
    b = serve(plane(), io, headers_match=True)
    try:
        conversations(b)
    finally:
        b.stop()


def test_refusals_leave_the_other_bindings_working(gpu):
    b = serve(plane(), "native", headers_match=True)
    try:
        assert (b.plane.hb_max, b.plane.hp_max) == (b.plane.info["hb_max"], b.plane.info["hp_max"]) == (8, 12)
        refusals(b)
    finally:
        b.stop()


def test_option_off_routes_as_topic(gpu):
    from chanamq_amd.client import Connection
    b = serve(plane(on=False), "native")
    try:
        c = Connection(port=b.port, vhost="/")
        ch = c.channel()
        ch.exchange_declare("hx", "headers")
        for q in QUEUES:
            ch.queue_declare(q)
            ch.queue_bind(q, "hx", "", BINDS[q])
        cc = c.channel()
        for q in QUEUES:
            cc.basic_consume(q, q, no_ack=True)
        publish_all(ch, "hx")
        assert collect(cc, len(QUEUES) * len(MESSAGES)) == EXPECTED_OFF
        c.close()
        assert b.plane.h_used == (0, 0)
    finally:
        b.stop()


def test_durable_bindings_survive_a_restart_with_their_arguments(gpu, tmp_path):
    from chanamq_amd.broker import load
    core = load()

    def boot():
        st = core.Store()
        st.open(str(tmp_path / "store"), True)
        p = plane(persist=1, persist_max=4096, persist_bytes=8 << 20, restore_max=1024, restore_bytes=8 << 20)
        return st, serve(p, "native", store=st, headers_match=True)
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
    finally:
        b.stop()
        st.close()
