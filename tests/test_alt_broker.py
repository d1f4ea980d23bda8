"""Alternate exchanges through the server: ``GpuBroker(alternate_exchange=True)`` on the golden
plane (CPU), spoken to by the AMQP test client.  tests/test_gpu_alt_broker.py runs the same
conversation on the HIP plane."""

import json
import urllib.request

import pytest

from alt_broker_script import ALT, alt_script
from test_xdeath_broker import golden, serve


@pytest.mark.parametrize("io", ["native", "python"])
def test_alternate_exchange_on_golden_plane(io):
    b = serve(golden(alternate_exchange=True), io, alternate_exchange=True)
    try:
        alt_script(b)
    finally:
        b.stop()


def test_admin_stats_serves_alt_routed():
    from chanamq_amd.server.admin import AdminServer
    b = serve(golden(alternate_exchange=True), alternate_exchange=True)
    admin = AdminServer(b, 0).start()
    try:
        with urllib.request.urlopen(f"http://127.0.0.1:{admin.port}/admin/stats", timeout=5) as r:
            assert json.loads(r.read())["alt_routed"] == 0
    finally:
        admin.stop()
        b.stop()


def test_broker_option_needs_a_plane_built_with_it():
    with pytest.raises(ValueError, match="alternate_exchange"):
        serve(golden(), alternate_exchange=True)


def test_off_the_argument_is_ignored_and_no_statistic_appears():
    from chanamq_amd.client import Connection
    b = serve(golden())
    try:
        c = Connection(port=b.port, vhost="/")
        ch = c.channel()
        ch.exchange_declare("ae", "fanout")
        ch.exchange_declare("front", "direct", arguments={ALT: "ae"})
        ch.exchange_declare("front", "direct", arguments={ALT: "other"})    # the unconditional no-op
        ch.queue_declare("catchall")
        ch.queue_bind("catchall", "ae", "")
        ch.confirm_select()
        ch.basic_publish("front", "missing", b"x", mandatory=True)
        assert ch.wait_for_confirms()
        assert [r.method.reply_code for r in ch.returns] == [312]
        assert "alt_routed" not in json.loads(b.stats_json())
        c.close()
    finally:
        b.stop()
