"""The consumer half of the step (k_chan_advance, the fused requeue, k_dequeue, runs_body,
k_dv_write, the delivery side of k_render) at the sizes where those kernels change path:
every scenario of tests/consumer_scenarios.py on the HIP data plane, judged by the client-side
statements of ``consumer_scenarios.CHECKS`` and compared byte by byte, step by step, with the
golden model.  The step-capacity trims (deliv_max, egress budget) have no golden model: their
test states what a client sees."""

import pytest

from consumer_scenarios import (CHECKS, FOLDED, SCENARIOS, body_of, ck_folded_settles_mixed, golden_plane, observe,
                                pubs, run_consumer, serial)
from dp_scenarios import VH
from e2e_scenarios import assert_same
from gpu_cfg import CFG

pytestmark = pytest.mark.gpu

MODES = {"graph": True, "eager": False}
_golden = {}


def golden_outs(name):
    """The golden model's run of a scenario: computed once, only read by the cases."""
    if name not in _golden:
        sc = SCENARIOS[name]
        g = golden_plane(dict(CFG, **sc.cfg))
        _golden[name] = run_consumer(g, sc.fn(g), sc.now_step_ms)
    return _golden[name]


def gpu_outs(sc, graph, **kw):
    from chanamq_amd.engine.dataplane import GpuDataPlane
    d = GpuDataPlane(graph=graph, **kw, **dict(CFG, **sc.cfg))
    return d, run_consumer(d, sc.fn(d), sc.now_step_ms)


def compare(name, od):
    CHECKS[name](od)                    # what the clients must see, from the protocol
    og = golden_outs(name)
    assert_same(og, od)                 # and the model's bytes
    assert [o["counters"] for o in og] == [o["counters"] for o in od]


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_consumer_edges_match_golden(gpu, name, mode):
    d, od = gpu_outs(SCENARIOS[name], MODES[mode])
    compare(name, od)
    if name.startswith("requeue") or name in ("many_settles", "ttl_waves"):   # everything acked or expired
        assert d.last_counters["n_live_msgs"] == 0 and d.last_counters["live_bytes"] == 0


@pytest.mark.parametrize("mode", sorted(MODES))
def test_consumer_frame_max_bodies_inline(gpu, mode):
    """The same deliveries with egress by reference off: every body rendered into the egress
    by the device (the default renders the same step's bodies of 256 B up to one frame by
    reference; longer or shorter ones, and everything served from the backlog, inline)."""
    d, od = gpu_outs(SCENARIOS["consumer_frame_max"], MODES[mode], egress_ref=None)
    compare("consumer_frame_max", od)


def test_consumer_frame_max_reference_split(gpu):
    """By reference exactly the two bodies that fill at most one frame of the consumer's
    connection and are no shorter than ref_min: fm - 9 and fm - 8 bytes."""
    from chanamq_amd.engine.dataplane import GpuDataPlane
    from consumer_scenarios import FM
    sc = SCENARIOS["consumer_frame_max"]
    d = GpuDataPlane(**CFG)
    steps = sc.fn(d)
    r = d.step(steps[0])
    assert r.counters["n_ref"] == 2 and r.counters["ref_bytes"] == (FM - 9) + (FM - 8)


@pytest.mark.parametrize("mode", sorted(MODES))
def test_folded_settles_mixed(gpu, mode):
    """More than MS_MAX multiple settles whose tail mixes acks and requeues: the engine folds
    the tail (PARITY.md), so no byte comparison; nothing is lost, nothing doubled without the
    flag, and every message is released once all are acked."""
    d, od = gpu_outs(FOLDED, MODES[mode])
    ck_folded_settles_mixed(od)
    assert d.last_counters["n_live_msgs"] == 0


# ---------------------------------------------------------------- step-capacity trims
TRIM_BODY = 16
TRIM_CONS = ((2, "a"), (3, "b"), (4, "c"))


def trim_plane(**over):
    from chanamq_amd.engine.dataplane import GpuDataPlane
    d = GpuDataPlane(**dict(CFG, **over))
    d.declare_queue(VH, "cq")
    d.open_connection(1, VH)
    d.open_channel(1, 1)
    return d


def trim_attach(d, prefetch):
    for conn, tag in TRIM_CONS:
        d.open_connection(conn, VH)
        d.open_channel(conn, 1)
        d.qos(conn, 1, prefetch_count=prefetch)
        d.consume(conn, 1, VH, "cq", tag, no_ack=False)


def trim_pubs(lo, hi):
    from chanamq_amd.engine.traffic import publish_command
    return b"".join(publish_command(1, "", "cq", body_of("cq", i, TRIM_BODY)) for i in range(lo, hi))


def trim_drain(d, total, per_step, first=None):
    """Step until ``total`` messages are out, acking everything before each step but the
    first; per step exactly min(per_step, what is left), the next stretch of the queue."""
    from chanamq_amd.engine.traffic import ack_frame
    outs, done, k = [], 0, 0
    holders = set()
    while done < total:
        assert k < 8, "the backlog does not drain"
        r = d.step({c: ack_frame(1, 0, multiple=True) for c in sorted(holders)})
        outs.append(dict(egress=r.egress))
        seen = [s for s in observe(outs) if s.step == k]
        got = [serial(s.body)[1] for s in seen]
        assert len(got) == min(per_step, total - done), f"step {k}: {len(got)} deliveries"
        assert sorted(got) == list(range(done, done + len(got))), f"step {k}: not the head of the queue"
        if k == 0 and first is not None:
            assert [(s.ctag, serial(s.body)[1]) for s in seen] == first
        holders |= {s.conn for s in seen}
        done += len(got)
        k += 1
    seen = observe(outs)
    for conn, tag in TRIM_CONS:      # tags count up per channel, each consumer sees the queue's order
        mine = [s for s in seen if s.conn == conn]
        assert [s.tag for s in mine] == list(range(1, len(mine) + 1))
        assert [serial(s.body)[1] for s in mine] == sorted(serial(s.body)[1] for s in mine)
        assert all(s.ctag == tag and not s.redelivered for s in mine)
    assert sorted(serial(s.body)[1] for s in seen) == list(range(total))       # each exactly once
    r = d.step({c: ack_frame(1, 0, multiple=True) for c in sorted(holders)})
    assert r.counters["n_deliv"] == 0 and r.counters["n_live_msgs"] == 0 and r.counters["live_bytes"] == 0


def trim_credit_back(d, n):
    """With a and b cancelled, c alone takes n <= prefetch new messages in one step: the
    credit and the window slots of the grants that were trimmed away came back."""
    from chanamq_amd.engine.traffic import ack_frame
    d.cancel(2, 1, "a")
    d.cancel(3, 1, "b")
    r = d.step({1: trim_pubs(1000, 1000 + n)})
    seen = observe([dict(egress=r.egress)])
    assert [(s.conn, serial(s.body)[1]) for s in seen] == [(4, 1000 + i) for i in range(n)]
    r = d.step({4: ack_frame(1, 0, multiple=True)})
    assert r.counters["n_live_msgs"] == 0


def test_step_capacity_trims_delivery_slots(gpu):
    """deliv_max 256, a backlog of 400, three manual-ack consumers with prefetch 200: the
    grants are 134 + 133 + 133, and the step has 256 delivery slots.  The trim takes from
    the last run backwards: a keeps 134, b 122, c none -- the first 256 of the queue, in
    order.  The rest follows; the trimmed credit is not lost."""
    d = trim_plane(deliv_max=256)
    assert d.step({1: trim_pubs(0, 400)}).counters["n_deliv"] == 0
    trim_attach(d, 200)
    first = [("a", i) for i in range(134)] + [("b", i) for i in range(134, 256)]
    trim_drain(d, 400, 256, first)
    trim_credit_back(d, 200)


def test_step_capacity_trims_egress_budget(gpu):
    """The same backlog under an egress budget of 8192 bytes a step: a step keeps the longest
    prefix of the granted entries whose frames fit -- floor(8192 / size of one rendered
    Basic.Deliver) -- all on the first consumer of the walk."""
    from chanamq_amd.protocol.codec import Method, render_command
    cap = 8192
    one = len(render_command(1, Method("basic.deliver", consumer_tag="a", delivery_tag=1, redelivered=False,
                                       exchange="", routing_key="cq"), {}, body_of("cq", 0, TRIM_BODY)))
    keep = cap // one
    assert 64 < keep < 134        # the budget cuts inside the first run (134), before the slot trim could
    d = trim_plane(egress_cap=cap)
    assert d.step({1: trim_pubs(0, 400)}).counters["n_deliv"] == 0
    trim_attach(d, 200)
    trim_drain(d, 400, keep, [("a", i) for i in range(keep)])
    trim_credit_back(d, keep)
