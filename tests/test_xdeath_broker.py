"""x-death headers and cycle detection through the server: ``GpuBroker(dead_letter=True,
x_death=True)`` on the golden plane (CPU), spoken to by the AMQP test client.
tests/test_gpu_xdeath_broker.py runs the same conversation on the HIP plane."""

import json
import urllib.request

import pytest

from xdeath_broker_script import xdeath_script

SMALL = dict(c_max=64, chpc=8, q_max=64, x_max=64, cons_max=256, ucap=256, deliver_cap=4096)


def golden(**kw):
    from chanamq_amd.engine.golden import GoldenDataPlane
    return GoldenDataPlane(default_queue_capacity=1 << 12, ring_pool=1 << 20, **dict(SMALL, **kw))


def serve(plane, io="python", **kw):
    from chanamq_amd.server.gpu_broker import GpuBroker
    return GpuBroker(plane, idle_step_ms=1.0, io=io, ingress_bytes=8 << 20, **kw).start()


@pytest.mark.parametrize("io", ["native", "python"])
def test_x_death_on_golden_plane(io):
    b = serve(golden(dead_letter=True, x_death=True), io, dead_letter=True, x_death=True)
    try:
        xdeath_script(b)
    finally:
        b.stop()


def test_admin_stats_serves_dl_cycle():
    from chanamq_amd.server.admin import AdminServer
    b = serve(golden(dead_letter=True, x_death=True), dead_letter=True, x_death=True)
    admin = AdminServer(b, 0).start()
    try:
        with urllib.request.urlopen(f"http://127.0.0.1:{admin.port}/admin/stats", timeout=5) as r:
            assert json.loads(r.read())["dl_cycle"] == 0
    finally:
        admin.stop()
        b.stop()


def test_broker_option_needs_dead_letter_and_a_plane_built_with_it():
    with pytest.raises(ValueError, match="dead_letter"):
        serve(golden(dead_letter=True, x_death=True), x_death=True)
    with pytest.raises(ValueError, match="x_death"):
        serve(golden(dead_letter=True), dead_letter=True, x_death=True)
