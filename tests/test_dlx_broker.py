"""Dead-lettering through the server: ``GpuBroker(dead_letter=True)`` on the golden plane (CPU),
spoken to by the AMQP test client.  tests/test_gpu_dlx_broker.py runs the same conversations on
the HIP plane."""

import json
import urllib.request

import pytest

from dlx_broker_script import DL_STATS, dlx_script, off_script, refusals_script

SMALL = dict(c_max=64, chpc=8, q_max=64, x_max=64, cons_max=256, ucap=256, deliver_cap=4096)


def golden(on=True, **kw):
    from chanamq_amd.engine.golden import GoldenDataPlane
    return GoldenDataPlane(default_queue_capacity=1 << 12, ring_pool=1 << 20, **dict(SMALL, **kw),
                           **({"dead_letter": True} if on else {}))


def serve(plane, io="python", **kw):
    from chanamq_amd.server.gpu_broker import GpuBroker
    return GpuBroker(plane, idle_step_ms=1.0, io=io, ingress_bytes=8 << 20, **kw).start()


@pytest.mark.parametrize("io", ["native", "python"])
def test_dead_letter_on_golden_plane(io):
    b = serve(golden(), io, dead_letter=True)
    try:
        dlx_script(b)
    finally:
        b.stop()


def test_invalid_arguments_are_406():
    b = serve(golden(), dead_letter=True)
    try:
        refusals_script(b)
    finally:
        b.stop()


def test_admin_stats_serves_the_counters():
    from chanamq_amd.server.admin import AdminServer
    b = serve(golden(), dead_letter=True)
    admin = AdminServer(b, 0).start()
    try:
        with urllib.request.urlopen(f"http://127.0.0.1:{admin.port}/admin/stats", timeout=5) as r:
            s = json.loads(r.read())
        assert all(s[k] == 0 for k in DL_STATS)
    finally:
        admin.stop()
        b.stop()


def test_option_off_ignores_the_arguments():
    b = serve(golden(on=False))
    try:
        off_script(b)
    finally:
        b.stop()


def test_broker_option_needs_a_plane_built_with_it():
    with pytest.raises(ValueError):
        serve(golden(on=False), dead_letter=True)


def test_config_keys_reach_plane_and_broker(tmp_path):
    from chanamq_amd.utils.config import Config
    plane, broker = Config.load([], {}).gpu_config()
    assert broker["dead_letter"] is False and "dead_letter" not in plane
    f = tmp_path / "on.conf"
    f.write_text("chana.mq.gpu.dead-letter = true\nchana.mq.gpu.dead-max = 256\nchana.mq.gpu.dead-bytes = 65536\n")
    plane, broker = Config.load([str(f)], {}).gpu_config(single=True)
    assert broker["dead_letter"] is True
    assert (plane["dead_letter"], plane["dead_max"], plane["dead_bytes"]) == (True, 256, 65536)
