"""Priority queues through the server: ``GpuBroker(priority_queues=True)`` on the golden plane
(CPU), spoken to by the AMQP test client.  tests/test_gpu_prio_broker.py runs the same
conversations on the HIP plane."""

import json
import urllib.request

import pytest

from prio_broker_script import off_script, priority_script, refusals_script

SMALL = dict(c_max=64, chpc=8, q_max=64, x_max=64, cons_max=256, ucap=256, deliver_cap=4096)
ON = dict(priority_queues=True)


def golden(on=True, **kw):
    from chanamq_amd.engine.golden import GoldenDataPlane
    return GoldenDataPlane(default_queue_capacity=1 << 12, ring_pool=1 << 20, **dict(SMALL, **kw), **(ON if on else {}))


def serve(plane, io="python", **kw):
    from chanamq_amd.server.gpu_broker import GpuBroker
    return GpuBroker(plane, idle_step_ms=1.0, io=io, ingress_bytes=8 << 20, **kw).start()


@pytest.mark.parametrize("io", ["native", "python"])
def test_priorities_on_golden_plane(io):
    b = serve(golden(), io, **ON)
    try:
        priority_script(b)
    finally:
        b.stop()


def test_refusals_are_406():
    b = serve(golden(), **ON)
    try:
        refusals_script(b)
    finally:
        b.stop()


def test_refusals_beside_length_limits():
    lim = dict(queue_limits=True, queue_limit_bytes=True)
    b = serve(golden(**lim), **ON, **lim)
    try:
        refusals_script(b)
    finally:
        b.stop()


def test_admin_queues_serves_one_row_per_queue():
    from chanamq_amd.client import Connection
    from chanamq_amd.server.admin import AdminServer
    b = serve(golden(), **ON)
    admin = AdminServer(b, 0).start()
    try:
        c = Connection(port=b.port, vhost="/")
        ch = c.channel()
        ch.confirm_select()
        ch.queue_declare("a", arguments={"x-max-priority": 4})
        ch.queue_declare("u")
        for q in ("a", "u"):
            for p in (0, 4, 2, 4):
                ch.basic_publish("", q, b"abc", {"priority": p})
        assert ch.wait_for_confirms() is True
        c.close()
        with urllib.request.urlopen(f"http://127.0.0.1:{admin.port}/admin/queues", timeout=5) as r:
            got = json.loads(r.read())
        rows = {q["name"]: q for q in got}
        assert len(got) == 2
        assert [(rows[n]["ready"], rows[n]["max_priority"]) for n in ("a", "u")] == [(4, 4), (4, None)]
    finally:
        admin.stop()
        b.stop()


def test_flag_off_ignores_the_argument():
    b = serve(golden(on=False))
    try:
        off_script(b)
    finally:
        b.stop()


def test_flag_needs_a_plane_built_with_it():
    with pytest.raises(ValueError):
        serve(golden(on=False), **ON)
    b = serve(golden(on=False))
    try:
        assert b.priority_queues is False
    finally:
        b.stop()


def test_config_key_reaches_plane_and_broker(tmp_path):
    from chanamq_amd.utils.config import Config
    plane, broker = Config.load([], {}).gpu_config()
    assert broker["priority_queues"] is False and "priority_queues" not in plane
    f = tmp_path / "on.conf"
    f.write_text("chana.mq.gpu.priority-queues = true\n")
    plane, broker = Config.load([str(f)], {}).gpu_config()
    assert broker["priority_queues"] is True and plane["priority_queues"] is True
    plane, broker = Config.load([str(f)], {"chana.mq.gpu.priority-queues": "false"}).gpu_config()
    assert broker["priority_queues"] is False and "priority_queues" not in plane
