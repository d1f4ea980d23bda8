"""Queue byte limits through the server: ``GpuBroker(queue_limits=True, queue_limit_bytes=True)``
on the golden plane (CPU), spoken to by the AMQP test client.  tests/test_gpu_bytelimits_broker.py
runs the same conversations on the HIP plane."""

import json
import urllib.request

import pytest

from bytelimits_broker_script import bytelimits_script, off_script, refusals_script

SMALL = dict(c_max=64, chpc=8, q_max=64, x_max=64, cons_max=256, ucap=256, deliver_cap=4096)
ON = dict(queue_limits=True, queue_limit_bytes=True)


def golden(on=True, **kw):
    from chanamq_amd.engine.golden import GoldenDataPlane
    return GoldenDataPlane(default_queue_capacity=1 << 12, ring_pool=1 << 20, **dict(SMALL, **kw),
                           **(ON if on else {"queue_limits": True}))


def serve(plane, io="python", **kw):
    from chanamq_amd.server.gpu_broker import GpuBroker
    return GpuBroker(plane, idle_step_ms=1.0, io=io, ingress_bytes=8 << 20, **kw).start()


@pytest.mark.parametrize("io", ["native", "python"])
def test_bytelimits_on_golden_plane(io):
    b = serve(golden(), io, **ON)
    try:
        bytelimits_script(b)
    finally:
        b.stop()


def test_invalid_arguments_are_406():
    b = serve(golden(), **ON)
    try:
        refusals_script(b)
    finally:
        b.stop()


def test_admin_queues_serves_ready_bytes():
    from chanamq_amd.client import Connection
    from chanamq_amd.server.admin import AdminServer
    b = serve(golden(), **ON)
    admin = AdminServer(b, 0).start()
    try:
        c = Connection(port=b.port, vhost="/")
        ch = c.channel()
        ch.confirm_select()
        ch.queue_declare("a", arguments={"x-max-length-bytes": 7})
        ch.queue_declare("u")
        for q in ("a", "u"):
            for i in range(4):
                ch.basic_publish("", q, b"abc")
        assert ch.wait_for_confirms() is True
        c.close()
        with urllib.request.urlopen(f"http://127.0.0.1:{admin.port}/admin/queues", timeout=5) as r:
            rows = {q["name"]: q for q in json.loads(r.read())}
        assert [(rows[n]["ready"], rows[n]["ready_bytes"]) for n in ("a", "u")] == [(2, 6), (4, 12)]
    finally:
        admin.stop()
        b.stop()


def test_flag_off_ignores_the_argument():
    b = serve(golden(on=False), queue_limits=True)
    try:
        off_script(b)
    finally:
        b.stop()


def test_flag_needs_queue_limits_and_a_plane_built_with_it():
    from chanamq_amd.engine.golden import GoldenDataPlane
    with pytest.raises(ValueError):
        GoldenDataPlane(queue_limit_bytes=True, **SMALL)
    with pytest.raises(ValueError):
        serve(golden(), queue_limit_bytes=True)                        # the broker without queue_limits
    with pytest.raises(ValueError):
        serve(golden(on=False), **ON)                                  # a plane built without the flag
    b = serve(golden(on=False), queue_limits=True)
    try:
        assert b.queue_limit_bytes is False
    finally:
        b.stop()


def test_config_key_reaches_plane_and_broker(tmp_path):
    from chanamq_amd.utils.config import Config
    plane, broker = Config.load([], {}).gpu_config()
    assert broker["queue_limit_bytes"] is False and "queue_limit_bytes" not in plane
    f = tmp_path / "on.conf"
    f.write_text("chana.mq.gpu.queue-limits = true\nchana.mq.gpu.queue-limit-bytes = true\n")
    for single in (True, False):
        plane, broker = Config.load([str(f)], {}).gpu_config(single=single)
        assert broker["queue_limit_bytes"] is True and plane["queue_limit_bytes"] is True
    # the launcher's --set path: one key overridden on top of the files
    plane, broker = Config.load([str(f)], {"chana.mq.gpu.queue-limit-bytes": "false"}).gpu_config()
    assert broker["queue_limit_bytes"] is False and broker["queue_limits"] is True
    alone = tmp_path / "alone.conf"
    alone.write_text("chana.mq.gpu.queue-limit-bytes = true\n")
    with pytest.raises(ValueError):
        Config.load([str(alone)], {}).gpu_config()


def test_broker_from_a_config_file(tmp_path):
    """The flag from a config file, through ``gpu_config`` to a serving broker."""
    from chanamq_amd.utils.config import Config
    f = tmp_path / "on.conf"
    f.write_text("chana.mq.gpu.queue-limits = true\nchana.mq.gpu.queue-limit-bytes = true\n")
    plane, broker = Config.load([str(f)], {}).gpu_config()
    b = serve(golden(), queue_limits=broker["queue_limits"], queue_limit_bytes=broker["queue_limit_bytes"])
    try:
        assert b.queue_limit_bytes and plane["queue_limit_bytes"]
        refusals_script(b)
    finally:
        b.stop()
