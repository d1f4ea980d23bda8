"""Control operations staged while steps run (``GpuDataPlane.defer``: what the broker's light
sections do) on the HIP data plane against the golden model: the scenarios of
tests/deferred_scenarios.py byte by byte and step by step, the ``cons_active`` 2 -> 1 hand-over,
the methods that must refuse a device read under ``defer``, and a delta-carrying step submitted
behind steps still in flight."""

import numpy as np
import pytest

from consumer_scenarios import check_common, golden_plane, observe, per_step, serial
from deferred_scenarios import ACK_ALL, SCENARIOS, Shift, VH, light, pub, run_deferred, sc_third_consumer, stage_sections
from dp_scenarios import NOW
from e2e_scenarios import assert_same
from gpu_cfg import CFG

pytestmark = pytest.mark.gpu

MODES = {"graph": True, "eager": False}
_golden = {}


def golden_outs(name):
    """The golden model's run of a scenario: computed once, only read by the cases."""
    if name not in _golden:
        g = golden_plane(CFG)
        _golden[name] = run_deferred(g, SCENARIOS[name](g))
    return _golden[name]


def gpu_outs(fn, mode):
    from chanamq_amd.engine.dataplane import GpuDataPlane
    d = GpuDataPlane(graph=MODES[mode], **CFG)
    return d, run_deferred(d, fn(d))


def delivered(seen, n, **where):
    """Deliveries per step among those matching ``where`` (fields of ``Seen``)."""
    return per_step(seen, n, lambda s: all(getattr(s, k) == v for k, v in where.items()))


# what the clients must see in each scenario, from the protocol and the scenario's docstring
def ck_consume_handover(outs, seen):
    assert delivered(seen, 5, conn=2) == [0, 0, 8, 2, 0], "no delivery in the carrying step, the head in the next"
    assert [serial(s.body)[1] for s in seen] == list(range(10))


def ck_consume_cancel(outs, seen):
    assert {s.ctag for s in seen} == {"z"}, "a cancelled consumer took a delivery"
    assert delivered(seen, 8) == [0, 0, 0, 0, 0, 0, 12, 0]
    assert [serial(s.body)[1] for s in seen] == list(range(12))


def ck_flow(outs, seen):
    assert delivered(seen, 5) == [4, 0, 6, 2, 0]


def ck_qos(outs, seen):
    assert delivered(seen, 8) == [3, 2, 4, 0, 2, 1, 0, 0]


def ck_channel_close(outs, seen):
    assert [o["counters"]["n_requeue"] for o in outs] == [0, 3, 0, 0, 0]
    assert all(s.step == 0 for s in seen if s.conn == 2)
    again = [s for s in seen if s.redelivered]
    assert len(again) == 3 and all(s.step == 1 and s.conn == 3 for s in again)
    assert sorted(serial(s.body)[1] for s in seen if s.conn == 3) == sorted(list(range(10)))


def ck_connection_close(outs, seen):
    assert [o["counters"]["n_requeue"] for o in outs] == [0, 4, 0, 0, 0]
    assert all(s.step == 0 for s in seen if s.conn == 2)
    assert {s.ch for s in seen if s.conn == 2} == {1, 2}
    again = [s for s in seen if s.redelivered]
    assert len(again) == 4 and all(s.step == 1 and s.conn == 3 for s in again)


def ck_confirm_select(outs, seen):
    from chanamq_amd.protocol.codec import FrameParser, decode_method
    acks = []
    for o in outs:
        ms = [decode_method(f.payload) for f in FrameParser().feed(o["egress"].get(1, b"")) if f.type == 1]
        assert all(m.name == "basic.ack" for m in ms)
        acks.append([(m.delivery_tag, bool(m.multiple)) for m in ms])
    assert acks[0] == [] and acks[3] == []
    # confirm tags count from the Confirm.Select: step 1's three publishes are 1..3, step 2's is 4
    covered = lambda a: max((t for t, _ in a), default=0)
    assert covered(acks[1]) == 3 and covered(acks[2]) == 4


def ck_topology(outs, seen):
    assert delivered(seen, 7, ctag="t") == [2, 3, 1, 0, 0, 0, 0]
    assert delivered(seen, 7, ctag="new") == [0, 0, 0, 0, 0, 4, 0]


def ck_two_sections_one_step(outs, seen):
    assert delivered(seen, 5, conn=2) == [2, 1, 3, 0, 0]      # prefetch 3 from step 1 on, one ack of all
    assert delivered(seen, 5, conn=3) == [2, 0, 0, 2, 0]


def ck_same_row_twice(outs, seen):
    assert delivered(seen, 6) == [2, 1, 5, 2, 0, 0]


CHECKS = {name[3:]: fn for name, fn in list(globals().items()) if name.startswith("ck_")}
assert sorted(CHECKS) == sorted(SCENARIOS)


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_deferred_ops_match_golden(gpu, name, mode):
    """Every scenario: what the clients must see, then egress, ctrl, events, segs and the
    counters byte for byte against the golden model with the consume shift."""
    og = golden_outs(name)
    CHECKS[name](og, observe(og))            # (the model itself meets the statements)
    d, od = gpu_outs(SCENARIOS[name], mode)
    seen = observe(od)
    check_common(seen)
    CHECKS[name](od, seen)
    assert_same(og, od)
    assert [o["counters"] for o in og] == [o["counters"] for o in od]
    assert od[-1]["pending"] == (0, 0, 0)
    if name == "two_sections_one_step":
        assert od[1]["pending"] == (0, 0, 0), "two disjoint sections did not ride one step"
    if name == "same_row_twice":
        # channel_changed writes five 4-byte fields of the row: the second section's are left
        assert od[1]["pending"] == (5, 20, 0) and od[2]["pending"] == (0, 0, 0)


@pytest.mark.parametrize("mode", sorted(MODES))
def test_third_consumer_staged_mid_stream(gpu, mode):
    """Three consumers on one queue, the third staged before step 1: every message is delivered
    exactly once, each consumer sees the queue's order, the new one gets nothing in the carrying
    step and something afterwards, and tags count up from 1.  (No byte comparison: the
    round-robin walk counts the consumer that is not active yet, the golden shift does not.)"""
    d, od = gpu_outs(sc_third_consumer, mode)
    seen = observe(od)
    check_common(seen)                       # tags from 1 on each channel, no redelivery
    assert sorted(serial(s.body)[1] for s in seen) == list(range(24))
    for tag in "abc":
        mine = [serial(s.body)[1] for s in seen if s.ctag == tag]
        assert mine == sorted(mine) and mine, tag
    assert delivered(seen, 5, ctag="c")[:2] == [0, 0]
    assert delivered(seen, 5, ctag="c")[2] > 0
    assert delivered(seen, 5) == [6, 6, 6, 6, 0]


def test_device_reads_are_refused_under_defer(gpu):
    """Under ``defer`` every method that would read the device raises and stages nothing."""
    from chanamq_amd.engine.control import ControlError
    from chanamq_amd.engine.dataplane import GpuDataPlane
    from chanamq_amd.protocol import constants as C

    d = GpuDataPlane(**CFG)
    d.declare_queue(VH, "dq")
    for c in (1, 2):
        d.open_connection(c, VH)
        d.open_channel(c, 1)
    d.consume(2, 1, VH, "dq", "d", no_ack=False)
    r = d.step({1: pub("dq", 0, 3)})
    assert r.counters["n_deliv"] == 3
    assert d.reserve_ring_chunk(CFG["default_queue_capacity"]) == CFG["default_queue_capacity"]
    with light(d):
        d.declare_queue(VH, "fits")                      # the reserved chunk's one ring
        staged = d.deltas_pending()
        assert staged[0] > 0
        reads = [lambda: d.apply_ack(2, 1, 1), lambda: d.apply_ack(2, 1, 2, requeue=True, kind="nack"),
                 lambda: d.apply_ack(2, 1, 3, requeue=False, kind="reject"), lambda: d.recover(2, 1),
                 lambda: d.take_carry(1)]
        for k, read in enumerate(reads):
            with pytest.raises(RuntimeError, match="deferred"):
                read()
            assert d.deltas_pending() == staged, f"read {k} staged something"
        with pytest.raises(ControlError) as e:
            d.declare_queue(VH, "no_ring_left")
        assert e.value.code == C.RESOURCE_ERROR
        assert d.deltas_pending() == staged
        assert (VH, "no_ring_left") not in d.queues
    d.step({})
    assert d.deltas_pending() == (0, 0, 0)
    # between sections the same calls work: the three deliveries settle as asked
    d.apply_ack(2, 1, 1)
    d.apply_ack(2, 1, 2, requeue=True, kind="nack")
    r = d.step({})
    assert r.counters["n_requeue"] == 1


# ---------------------------------------------------------------- behind a step in flight
PIPE_STEPS = 13


def pipe_plane(cls, **kw):
    d = cls(**kw)
    d.declare_queue(VH, "pq")
    for c in (0, 1):
        d.open_connection(c, VH)
        d.open_channel(c, 1)
    d.consume(1, 1, VH, "pq", "c0", no_ack=False)
    return d


def pipe_consume(tag):
    return ("consume", (1, 1, VH, "pq", tag), dict(no_ack=False))


# one light section staged before each step (None: nothing); the consumer's connection acks
# everything in every step but the one its channel is closed in
PIPE_SCHEDULE = [None,
                 [("cancel", (1, 1, "c0"))],
                 [pipe_consume("c1")],
                 [("flow", (1, 1, False))],
                 [("flow", (1, 1, True))],
                 [("qos", (1, 1, 4))],
                 None,
                 [("close_channel", (1, 1))],
                 [("open_channel", (1, 1)), ("qos", (1, 1, 6)), pipe_consume("c2")],
                 [("qos", (1, 1, 3))],
                 [("cancel", (1, 1, "c2"))],
                 [pipe_consume("c3")],
                 None]
PIPE_CLOSED = {7}
assert len(PIPE_SCHEDULE) == PIPE_STEPS


def pipe_inputs(k):
    inp = {0: pub("pq", 8 * k, 8 * k + 8, size=64)}
    if k not in PIPE_CLOSED:
        inp[1] = ACK_ALL
    return inp


def nonempty(egress):
    return {c: bytes(b) for c, b in egress.items() if len(b)}


@pytest.fixture(scope="module")
def pipe_golden():
    """The golden run of the schedule (with the consume shift): computed once, only read."""
    g = pipe_plane(lambda: golden_plane(CFG))
    shift = Shift(g)
    want = []
    for k in range(PIPE_STEPS):
        if PIPE_SCHEDULE[k]:
            shift.apply([PIPE_SCHEDULE[k]])
        want.append(nonempty(g.step(pipe_inputs(k), now_ms=NOW + k)["egress"]))
        shift.after_step()
    assert sum(1 for w in want if w.get(1)) >= 6      # (the schedule leaves deliveries to compare)
    return want


def pipe_variants():
    from test_gpu_dataplane import PIPELINED
    return {k: PIPELINED[k] for k in ("overlap-prefetch", "par3", "hsa-par3")}


@pytest.mark.parametrize("variant", ["hsa-par3", "overlap-prefetch", "par3"])
def test_delta_steps_behind_steps_in_flight(gpu, variant, pipe_golden):
    """``parities`` steps outstanding (submit_raw / finish) over 13 steps -- one wrap of the
    parity, ingress and egress rotations -- with one light section staged between submits, while
    the steps before are still in flight: cancel, consume under a new tag, flow off and on, a
    prefetch change, close and reopen of the channel holding unacked messages.  Every step's
    egress, for every connection, equals the golden run of the same schedule with the consume
    shift.

    This test cannot prove the ordering of a delta-carrying step behind the routing half of the
    step before it, or that the 2 -> 1 flip of cons_active belongs in k_post: a run in which
    the kernels happen not to overlap passes without either.  It fails if the wait or the flip
    is lost and the overlap then changes what a step reads."""
    from chanamq_amd.engine.dataplane import GpuDataPlane
    from chanamq_amd.engine.layout import SEG_IN
    from test_gpu_dataplane import INGRESS_SLOTS

    graph, cfg, ahead = pipe_variants()[variant]
    d = pipe_plane(GpuDataPlane, graph=graph, **cfg, **CFG)
    if cfg.get("parities") == 3:
        assert d.info["parities"] == 3
    if cfg.get("h2d_hsa") and d.info["h2d_hsa_engine"] < 0:
        pytest.skip("no HSA copy engine for the ingress on this device")
    inputs = [pipe_inputs(k) for k in range(PIPE_STEPS)]
    # each step's segments in their own 16-byte-aligned region of one page-locked pool
    region = max(sum((len(b) + 15) & ~15 for b in inp.values()) for inp in inputs)
    pool = d.mod.alloc_pinned(region * PIPE_STEPS)
    assert pool.ctypes.data % 16 == 0
    segs, plen = [], []
    for k, inp in enumerate(inputs):
        sg = np.zeros(len(inp), SEG_IN)
        off = 0
        for j, c in enumerate(sorted(inp)):
            pool[k * region + off:k * region + off + len(inp[c])] = np.frombuffer(inp[c], np.uint8)
            sg[j] = (c, len(inp[c]), off)
            off += (len(inp[c]) + 15) & ~15
        segs.append(sg)
        plen.append(off)
    ptr = lambda k: pool.ctypes.data + k * region
    queued, submitted, finished = [-1], [0], [-1]

    def prefetch_ahead():
        for t in range(submitted[0], min(submitted[0] + ahead, PIPE_STEPS)):
            if t > queued[0] and t - INGRESS_SLOTS <= finished[0]:
                assert d.prefetch(ptr(t), plen[t]) is True, f"prefetch of step {t}"
                queued[0] = t

    tickets = {}

    def submit(k):
        tickets[k] = d.submit_raw(segs[k], ptr(k), plen[k], now_ms=NOW + k)
        submitted[0] = k + 1
        prefetch_ahead()
        # the next step's section, staged while this one (and the ones before) are in flight
        if k + 1 < PIPE_STEPS and PIPE_SCHEDULE[k + 1]:
            stage_sections(d, [PIPE_SCHEDULE[k + 1]])

    assert PIPE_SCHEDULE[0] is None
    prefetch_ahead()
    for k in range(d.parities - 1):
        submit(k)
    for k in range(PIPE_STEPS):
        if k + d.parities - 1 < PIPE_STEPS:
            submit(k + d.parities - 1)
        r = d.finish(tickets.pop(k))
        finished[0] = k
        prefetch_ahead()
        assert nonempty(r.egress) == pipe_golden[k], f"step {k} egress differs"
    assert d.deltas_pending() == (0, 0, 0)
