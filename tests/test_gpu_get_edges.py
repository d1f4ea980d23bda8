"""Basic.Get between steps on the HIP data plane (k_basic_get and the host's GET_RETRY / GET_COLD
loop in GpuDataPlane.basic_get): every scenario of tests/get_scenarios.py, in the captured
graph and with eager launches, judged by the scenarios' client-side ``CHECKS`` and then compared
with the golden model step by step -- the Gets' frames and message-counts, egress, events,
counters, queue depths and ready bytes before and after each step, the store records of a
persisting plane, and the live messages and log bytes.

The Get buffer has no golden model: its case states what a client sees, at the one body size
that fits the buffer and the first that does not."""

import pytest
import torch  # noqa: F401  (loaded before the extension initialises HIP)

pytest.register_assert_rewrite("get_scenarios", "tier_scenarios")   # (their checks report what they compared)

from consumer_scenarios import body_of, observe
from dp_scenarios import NOW, VH
from e2e_scenarios import assert_same
from get_scenarios import CHECKS, SCENARIOS, assert_same_get, decode_get, golden_plane, gpu_plane, run_get
from gpu_cfg import CFG

pytestmark = pytest.mark.gpu

MODES = {"graph": True, "eager": False}
_golden = {}


def golden_outs(name):
    """The golden model's run of a scenario: computed once, only read by the cases."""
    if name not in _golden:
        sc = SCENARIOS[name]
        g = golden_plane(dict(CFG, **sc.cfg))
        _golden[name] = run_get(g, sc.fn(g), sc.now_step_ms)
    return _golden[name]


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_get_edges_match_golden(gpu, name, mode):
    sc = SCENARIOS[name]
    d = gpu_plane(dict(CFG, **sc.cfg), MODES[mode])
    od = run_get(d, sc.fn(d), sc.now_step_ms)
    CHECKS[name](od)                    # what the clients must see, from the protocol
    og = golden_outs(name)
    assert_same(og, od)                 # the model's bytes: frames and counts of every Get, egress, events
    assert_same_get(og, od)


@pytest.mark.parametrize("mode", sorted(MODES))
def test_get_buffer(gpu, mode):
    """The Get buffer holds carry_cap + carry_cap / 64 + 4096 bytes (270 336 with the test config's
    carry_cap of 256 KiB).  A publish on the wire is bounded by the connection's carry, so no wire
    publish exceeds it; a host-assembled one (publish_host, the path of messages larger than the
    carry) does.  GetOk (21 bytes of method for exchange "" and a 2-byte key), the header (12 + 2
    bytes of properties) and three body frames (frame-max 131 072) cost 75 bytes of framing, so
    a body of cap - 75 bytes fits exactly and one byte more does not: that Get raises
    RESOURCE_ERROR on 60/70, takes no delivery tag, the message stays at the head with the one
    behind it, and a consumer attached afterwards receives both intact."""
    from chanamq_amd.engine.control import ControlError
    from chanamq_amd.engine.traffic import publish_command
    from chanamq_amd.protocol.codec import encode_properties
    d = gpu_plane(dict(CFG), MODES[mode])
    cap = d.info["carry_cap"] + d.info["carry_cap"] // 64 + 4096
    assert cap == 270336 and d.max_host_message() > cap
    fit = cap - (8 + 21) - (8 + 12 + 2) - 3 * 8
    assert 2 * (131072 - 8) < fit <= 3 * (131072 - 8)
    for q in ("ga", "gb"):
        d.declare_queue(VH, q)
    for conn in (1, 2, 3):
        d.open_connection(conn, VH)
        d.open_channel(conn, 1)
    bodies = {"ga": [body_of("ga", 0, fit)], "gb": [body_of("gb", 0, fit + 1), body_of("gb", 1, 50)]}
    x = d.exchanges[(VH, "")].slot
    for q in bodies:
        for b in bodies[q]:
            assert d.publish_host(1, 1, x, b"", q.encode(), encode_properties({}), b, 0, now_ms=NOW) == 1
    slot = {q: d.queues[(VH, q)].slot for q in bodies}
    assert {q: d.message_count(slot[q]) for q in bodies} == {"ga": 1, "gb": 2}, "the publishes were not stored"
    g = decode_get(d.basic_get(2, 1, slot["ga"], True, now_ms=NOW))
    assert (g.tag, g.count, g.frames) == (1, 0, [131064, 131064, fit - 2 * 131064]) and g.body == bodies["ga"][0]
    with pytest.raises(ControlError) as e:
        d.basic_get(2, 1, slot["gb"], True, now_ms=NOW)
    assert (e.value.code, e.value.class_id, e.value.method_id) == (506, 60, 70)
    assert d.message_count(slot["gb"]) == 2
    d.consume(3, 1, VH, "gb", "c", no_ack=True)
    outs = [dict(egress=d.step({}, now_ms=NOW + k).egress) for k in (1, 2)]
    assert [(s.conn, s.tag, s.body) for s in observe(outs)] == [(3, 1, bodies["gb"][0]), (3, 2, bodies["gb"][1])]
    assert d.last_counters["n_live_msgs"] == 0 and d.last_counters["live_bytes"] == 0
    d.step({1: publish_command(1, "", "ga", body_of("ga", 1, 20))}, now_ms=NOW + 3)
    g = decode_get(d.basic_get(2, 1, slot["ga"], True, now_ms=NOW + 3))
    assert (g.tag, g.body) == (2, body_of("ga", 1, 20)), "the refused Get took a delivery tag"


@pytest.mark.parametrize("mode", sorted(MODES))
def test_get_buffer_ready_bytes(gpu, mode):
    """queue_limit_bytes on, and the buffer-too-small exit behind a skip: three expired bodies (100,
    200 and 300 bytes) ahead of a host-assembled body one byte too long for the Get buffer, and a
    50-byte body behind it.  The Get raises RESOURCE_ERROR on 60/70; the skip still happened, so
    two messages remain and ``queue_bytes`` is exactly the oversize body plus the one behind it;
    after a consumer drained the queue it is 0."""
    from chanamq_amd.engine.control import ControlError
    from chanamq_amd.engine.traffic import publish_command
    from chanamq_amd.protocol.codec import encode_properties
    d = gpu_plane(dict(CFG, queue_limits=True, queue_limit_bytes=True), MODES[mode])
    cap = d.info["carry_cap"] + d.info["carry_cap"] // 64 + 4096
    over = cap - (8 + 21) - (8 + 12 + 2) - 3 * 8 + 1
    d.declare_queue(VH, "gb", max_length_bytes=1 << 20)
    for conn in (1, 2, 3):
        d.open_connection(conn, VH)
        d.open_channel(conn, 1)
    slot = d.queues[(VH, "gb")].slot
    dead = [body_of("gb", i, n) for i, n in enumerate((100, 200, 300))]
    d.step({1: b"".join(publish_command(1, "", "gb", b, {"expiration": "1000"}) for b in dead)}, now_ms=NOW)
    x = d.exchanges[(VH, "")].slot
    live = [body_of("gb", 10, over), body_of("gb", 11, 50)]
    for b in live:
        assert d.publish_host(1, 1, x, b"", b"gb", encode_properties({}), b, 0, now_ms=NOW) == 1
    assert (d.message_count(slot), d.queue_bytes(slot)) == (5, 600 + over + 50)
    with pytest.raises(ControlError) as e:
        d.basic_get(2, 1, slot, True, now_ms=NOW + 2000)
    assert (e.value.code, e.value.class_id, e.value.method_id) == (506, 60, 70)
    assert (d.message_count(slot), d.queue_bytes(slot)) == (2, over + 50)
    d.consume(3, 1, VH, "gb", "c", no_ack=True)
    outs = [dict(egress=d.step({}, now_ms=NOW + 2000 + k).egress) for k in (1, 2)]
    assert [(s.conn, s.tag, s.body) for s in observe(outs)] == [(3, 1, live[0]), (3, 2, live[1])]
    assert (d.message_count(slot), d.queue_bytes(slot)) == (0, 0)
    assert d.last_counters["n_live_msgs"] == 0 and d.last_counters["live_bytes"] == 0
