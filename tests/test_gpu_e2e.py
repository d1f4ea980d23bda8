"""Exchange-to-exchange bindings on the HIP data plane: every scenario byte-identical to the
golden model, the random graph against the brute-force oracle, the Exchange.Bind
conversation over TCP, and 2- / 3-rank clusters against the single-plane oracle."""

import pytest

# (test_e2e_golden imports parallel.cluster, and with it torch, while this module is
# collected: torch's HIP runtime has to load before the data-plane extension's, as in
# test_gpu_sharded.py, or torch finds no device afterwards)
from e2e_scenarios import (SCENARIOS, assert_same, deliveries, publishes, run_e2e, sc_hundred, sc_random_graph,
                           sp_e2e_sharded, topology)
from test_e2e_golden import (assert_cluster_matches, conversation, expected_deliveries, golden, run_cluster_e2e,
                             run_single_e2e)

pytestmark = pytest.mark.gpu

from gpu_cfg import CFG  # noqa: E402


def gpu_plane(graph=True, **kw):
    from chanamq_amd.engine.dataplane import GpuDataPlane
    return GpuDataPlane(graph=graph, **dict(CFG, **kw))


@pytest.fixture(params=[True, False], ids=["graph", "eager"])
def graph(request):
    return request.param


@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_gpu_e2e_matches_golden(gpu, name, graph):
    g, d = golden(carry_cap=CFG["carry_cap"]), gpu_plane(graph)
    og = run_e2e(g, SCENARIOS[name](g))
    od = run_e2e(d, SCENARIOS[name](d))
    assert_same(og, od)
    assert any(o["egress"] for o in og)


def test_gpu_hundred_queues_behind_a_hop(gpu, graph):
    """Its own config (q_max 256): 100 queues behind a fanout hop, emit batches past 64 lanes."""
    cfg = dict(q_max=256, c_max=64, cons_max=256)
    g, d = golden(carry_cap=CFG["carry_cap"], **cfg), gpu_plane(graph, **cfg)
    og = run_e2e(g, sc_hundred(g))
    od = run_e2e(d, sc_hundred(d))
    assert_same(og, od)
    got = deliveries(od)
    assert len(got) == 100 and all(v == ["k", "k"] for v in got.values())


def test_gpu_random_graph_matches_oracle(gpu):
    d = gpu_plane()
    steps = sc_random_graph(d)
    topo = topology(d)
    assert deliveries(run_e2e(d, steps)) == expected_deliveries(topo, publishes(steps))


def test_gpu_bounds_come_from_the_engine(gpu):
    """The plane enforces the engine's own limits: HOP_QMAX / the slot bound as compiled, and
    topic rows that carry edges against tb_max, refused with 506 and nothing changed."""
    from chanamq_amd.engine.control import ControlError
    d = gpu_plane(tb_max=16)
    assert d.hop_qmax == d.info["hop_qmax"] >= 256 and d.hop_xslots == d.info["hop_xslots"] == 2048
    vh = "AMQ.DEFAULT"
    d.declare_exchange(vh, "t", "topic")
    d.declare_exchange(vh, "f", "fanout")
    for i in range(16):
        d.bind_exchange(vh, "f", "t", f"p{i}.*")
    with pytest.raises(ControlError) as e:
        d.bind_exchange(vh, "f", "t", "one.more")
    assert e.value.code == 506 and len(d.exchanges[(vh, "t")].xbindings) == 16


@pytest.mark.parametrize("io", ["native", "pipeline"])
def test_gpu_server_conversation(gpu, io):
    from chanamq_amd.engine.dataplane import GpuDataPlane
    from chanamq_amd.server.gpu_broker import GpuBroker
    from test_gpu_broker import GPU_CFG
    b = GpuBroker(GpuDataPlane(default_queue_capacity=1 << 12, **GPU_CFG), idle_step_ms=1.0, io=io,
                  ingress_bytes=8 << 20, exchange_bindings=True).start()
    try:
        conversation(b)
    finally:
        b.stop()


@pytest.mark.parametrize("world", [2, 3])
def test_gpu_cluster_matches_single_plane(gpu, world):
    import torch

    from chanamq_amd.engine.dataplane import GpuDataPlane
    torch.cuda.set_device(0)
    single = run_single_e2e(sp_e2e_sharded(), world)
    _, clus = run_cluster_e2e(sp_e2e_sharded(), world, lambda **kw: GpuDataPlane(**CFG, **kw))
    assert_cluster_matches(single, clus)


def test_gpu_walk_list_reservation_overflow(gpu):
    """pair_max 64 and walks of 25 / 40 queues: the step's hop_q reservations (and its pair
    table) do not hold them all.  A walk that does not fit is not enqueued and its publisher
    gets Basic.Nack; what is enqueued reaches each of its queues once; the next step, which
    fits, routes in full and is acked."""
    from chanamq_amd.protocol.codec import CommandAssembler, FrameParser
    from e2e_scenarios import sc_wide, stream
    d = gpu_plane(pair_max=64)
    steps = sc_wide(d)
    d.confirm_select(1, 1)
    fp, ca = FrameParser(), CommandAssembler()

    def step(data):
        r = d.step({1: data} if data else {})
        cmds = [c for fr in fp.feed(r.egress.get(1, b"")) for c in [ca.feed(fr)] if c is not None]
        return r, [c.method.name for c in cmds if c.method is not None], deliveries([dict(egress=r.egress)])
    r, replies, got = step(steps[0][1])                     # 12 publishes, 25 or 40 queues each
    n = sum(len(v) for v in got.values())
    assert r.counters["n_ring_full"] > 0 and "basic.nack" in replies
    assert 0 < n <= 64 and n == r.counters["n_pairs"]
    assert all(t.startswith("c-w") and len(v) <= 2 for t, v in got.items())   # at most two walks fit
    for key in ("k", "j"):                                  # a walk that fits reaches all of its queues
        copies = [v.count(key) for v in got.values() if key in v]
        assert len(copies) in (0, 40 if key == "k" else 25) and len(set(copies)) <= 1, (key, copies)
    r, replies, got = step(stream([("wa", "k")], seed=30))  # 40 pairs: fits
    assert r.counters["n_ring_full"] == 0 and replies == ["basic.ack"]
    assert len(got) == 40 and all(v == ["k"] for v in got.values())
