"""Queue length limits through the server: ``GpuBroker(queue_limits=True)`` on the golden plane
(CPU), spoken to by the AMQP test client.  tests/test_gpu_limits_broker.py runs the same
conversations on the HIP plane."""

import json
import urllib.request

import pytest

from limits_broker_script import durable_after, durable_before, limits_script, off_script, refusals_script

SMALL = dict(c_max=64, chpc=8, q_max=64, x_max=64, cons_max=256, ucap=256, deliver_cap=4096)


def golden(on=True, **kw):
    from chanamq_amd.engine.golden import GoldenDataPlane
    return GoldenDataPlane(default_queue_capacity=1 << 12, ring_pool=1 << 20, **dict(SMALL, **kw),
                           **({"queue_limits": True} if on else {}))


def serve(plane, io="python", **kw):
    from chanamq_amd.server.gpu_broker import GpuBroker
    return GpuBroker(plane, idle_step_ms=1.0, io=io, ingress_bytes=8 << 20, **kw).start()


@pytest.mark.parametrize("io", ["native", "python"])
def test_limits_on_golden_plane(io):
    b = serve(golden(), io, queue_limits=True)
    try:
        limits_script(b)
    finally:
        b.stop()


def test_invalid_arguments_are_406():
    b = serve(golden(), queue_limits=True)
    try:
        refusals_script(b)
    finally:
        b.stop()


def test_admin_stats_serves_both_counters():
    from chanamq_amd.client import Connection
    from chanamq_amd.server.admin import AdminServer
    b = serve(golden(), queue_limits=True)
    admin = AdminServer(b, 0).start()
    try:
        c = Connection(port=b.port, vhost="/")
        ch = c.channel()
        ch.confirm_select()
        ch.queue_declare("a", arguments={"x-max-length": 1})
        ch.queue_declare("r", arguments={"x-max-length": 1, "x-overflow": "reject-publish"})
        for q in ("a", "r"):
            for i in range(4):
                ch.basic_publish("", q, b"%d" % i)
        assert ch.wait_for_confirms() is False
        c.close()
        with urllib.request.urlopen(f"http://127.0.0.1:{admin.port}/admin/stats", timeout=5) as r:
            s = json.loads(r.read())
        assert (s["maxlen_dropped"], s["maxlen_rejected"]) == (3, 3)
    finally:
        admin.stop()
        b.stop()


def test_option_off_ignores_the_arguments():
    """(As before this option existed: the one conversation here that needs nothing of it.)"""
    b = serve(golden(on=False))
    try:
        off_script(b)
    finally:
        b.stop()


def test_broker_option_needs_a_plane_built_with_it():
    b = serve(golden(on=False))
    try:
        assert b.queue_limits is False
    finally:
        b.stop()
    with pytest.raises(ValueError):
        serve(golden(on=False), queue_limits=True)


def test_config_key_reaches_plane_and_broker(tmp_path):
    from chanamq_amd.utils.config import Config
    plane, broker = Config.load([], {}).gpu_config()
    assert broker["queue_limits"] is False and "queue_limits" not in plane
    f = tmp_path / "on.conf"
    f.write_text("chana.mq.gpu.queue-limits = true\n")
    for single in (True, False):
        plane, broker = Config.load([str(f)], {}).gpu_config(single=single)
        assert broker["queue_limits"] is True and plane["queue_limits"] is True


def test_recovered_durable_queue_adopts_a_limit(tmp_path):
    from chanamq_amd.broker import load
    core = load()

    def boot():
        st = core.Store()
        st.open(str(tmp_path / "store"), True)
        return st, serve(golden(persist=True), "python", store=st, queue_limits=True)
    st, b = boot()
    try:
        durable_before(b.port)
    finally:
        b.stop()
        st.close()
    st, b = boot()
    try:
        durable_after(b)
    finally:
        b.stop()
        st.close()


def test_reload_lifts_and_restores_the_limit():
    """``GpuPersistence._reload``: a reject-publish queue at its limit still takes a reload, and
    has its limit back afterwards."""
    from chanamq_amd.engine.persistence import GpuPersistence
    g = golden(persist=True)
    slot = g.declare_queue("AMQ.DEFAULT", "rq", durable=True, max_length=1, overflow="reject-publish")
    seen = []
    restore = g.restore
    g.restore = lambda items, now_ms=0: (seen.append(g.queue_by_slot[slot].max_length), restore(items, now_ms))[1]
    ps = GpuPersistence.__new__(GpuPersistence)
    ps.plane = g
    items = [(slot, 100 + i, 0, 0, b"", b"rq", b"", b"b%d" % i, True, False) for i in range(3)]
    assert ps._reload(items, 0) == 3 and seen == [None]
    q = g.queue_by_slot[slot]
    assert (q.max_length, q.overflow) == (1, "reject-publish") and g.message_count(slot) == 3
