"""Six consecutive pipelined steps on the three ways a step's end reaches the host -- one graph
(the bench's engine), one graph with persistence (k_host_out behind k_post), eager launches --
each with two steps in flight: what the host reads behind ``wait`` -- counters, segment
results, egress -- is that step's at every step, never the previous step's of the same IO set
(every step publishes a different number of messages, so a stale read shows).

The step-sequence word the issue planned for this test is not in the engine: that part of the
change was dropped (profiles/link_rate/summary.md), so the completion notice is the event on
all three paths and there is no word to compare with the sequence number."""

import pytest

from chanamq_amd.engine.traffic import publish_stream

pytestmark = pytest.mark.gpu

from gpu_cfg import CFG  # noqa: E402

VH = "AMQ.DEFAULT"
STEPS = 6
BASE = dict(copy_engine=3, overlap=0, h2d_hsa=1)
ENGINES = {
    "graph": dict(BASE, graph=True),
    "persist": dict(BASE, graph=True, persist=1, persist_max=4096, persist_bytes=8 << 20, restore_max=1024),
    "eager": dict(BASE, graph=False),
}


def topology(dp):
    """4 connections, 2 queues on a topic exchange: 1 and 2 publish, 3 and 4 consume."""
    dp.declare_exchange(VH, "nx", "topic")
    dp.declare_queue(VH, "na")
    dp.declare_queue(VH, "nb")
    dp.bind(VH, "na", "nx", "n.*")
    dp.bind(VH, "nb", "nx", "#.odd")
    for c in (1, 2, 3, 4):
        dp.open_connection(c, VH)
        dp.open_channel(c, 1)
    dp.consume(3, 1, VH, "na", "ca", no_ack=True)
    dp.consume(4, 1, VH, "nb", "cb", no_ack=True)


def step_inputs(k):
    """Step k publishes 3 (k + 1) messages: every step's counters differ from its neighbours'."""
    key = lambda i: "n.odd" if i % 2 else "n.even"
    return {1: publish_stream(2 * (k + 1), "nx", key, 200 + 16 * k, seed=20 + k),
            2: publish_stream(k + 1, "nx", key, 90, seed=40 + k)}


@pytest.fixture(scope="module")
def golden():
    from chanamq_amd.engine.golden import GoldenDataPlane

    g = GoldenDataPlane(c_max=CFG["c_max"], chpc=CFG["chpc"], q_max=CFG["q_max"], x_max=CFG["x_max"],
                        cons_max=CFG["cons_max"], ucap=CFG["ucap"], carry_cap=CFG["carry_cap"],
                        default_queue_capacity=CFG["default_queue_capacity"])
    topology(g)
    return [g.step(step_inputs(k), now_ms=1_800_000_000_000 + k) for k in range(STEPS)]


@pytest.mark.parametrize("kind", sorted(ENGINES))
def test_notice_every_step(gpu, golden, kind):
    from chanamq_amd.engine.dataplane import GpuDataPlane

    d = GpuDataPlane(**ENGINES[kind], **CFG)
    topology(d)
    seen = []

    def collect(t, k):
        d.wait(t)
        r = d.finish(t, waited=True)
        want = golden[k]
        assert r.counters["n_pubs"] == 3 * (k + 1), f"step {k} counters are another step's"
        assert r.counters["n_deliv"] == want["counters"]["n_deliv"], f"step {k} n_deliv"
        assert sorted(r.egress) == sorted(want["egress"]), f"step {k} egress conns"
        for c in want["egress"]:
            assert r.egress[c] == want["egress"][c], f"step {k} conn {c} egress differs"
        assert sorted(s[:4] for s in r.segs) == sorted(tuple(s[:4]) for s in want["segs"]), f"step {k} segs"
        seen.append(k)

    # two steps in flight, as the pipelined drivers run: step k is collected behind k + 1's submit
    pending = []
    for k in range(STEPS):
        segs, ptr, n = d.stage(step_inputs(k))
        pending.append((d.submit_raw(segs, ptr, n, now_ms=1_800_000_000_000 + k), k))
        if len(pending) > 1:
            collect(*pending.pop(0))
    collect(*pending.pop(0))
    assert seen == list(range(STEPS))
