"""The cross-rank pack / import / restore scenarios of tests/xchg_scenarios.py on a cluster of
golden planes (CPU), judged by the scenario's own record (``xchg_scenarios.check_run``: every
connection's egress rendered by the host codec from the topology, owners and traffic) and,
without a lag, compared byte for byte with one golden plane that holds every connection.  This
holds the model to the record, proves every placement assertion of the scenarios (they run
while a scenario is built) and shows that the inputs are sound.  The model's send buffers are
not in slot layout, so the direct check of the send buffers runs on the device only
(tests/test_gpu_xchg_edges.py), which also compares its bytes with this model's.

``many_tiles`` (66 561 publishes through Python) runs here too: building it takes 1.2 s and the
model's run of it 1.3 s on the CPU, in proportion to the rest of this file."""

import pytest

from gpu_cfg import CFG
from xchg_scenarios import (RECV_CFG, RESTORE_BYTES, RESTORE_MAX, SCENARIOS, SEND_CASES, SEND_CFG, assert_same_egress,
                            check_empty, check_run, golden_cluster, limits, restore_chunks, restore_items, restore_tuple,
                            restore_wire, run_net, single_oracle)

GOLDEN_COUNTERS = ("n_ring_full",)

# name -> [(world, scenario parameters, config overrides)]
CASES = {
    "many_tiles": [(2, {}, dict(cmd_max=65 * 1024 + 1))],
    "tile_edges": [(2, dict(prod=0), {}), (2, dict(prod=1), {}), (3, dict(prod=0), {}), (3, dict(prod=1), {})],
    "world_wide": [(8, {}, {}), (16, {}, {}), (8, dict(high_slots=True), dict(q_max=512)),
                   (16, dict(high_slots=True), dict(q_max=512)),
                   # a pair key one bit wider than SORT_ONEPASS_BITS: the several-pass sort at world > 1
                   (8, dict(high_slots=True), dict(q_max=1024)), (16, dict(high_slots=True), dict(q_max=1024))],
    "oneq_paths": [(3, {}, {})],
    "record_fields": [(2, {}, {})],
    "step_sequence": [(2, {}, {})],
    "recv_limits": [(3, {}, RECV_CFG)],
}
FLAT = [(n, w, tuple(sorted(p.items())), tuple(sorted(c.items()))) for n, cs in CASES.items() for w, p, c in cs]


def case_id(n, w, p, c, *more):
    return "-".join([n, f"w{w}"] + [f"{k}{v}" for k, v in p + c] + [str(m) for m in more])


def golden_run(name, world, params, over, lag):
    cfg = dict(CFG, **dict(over))
    net = SCENARIOS[name](golden_cluster(cfg, world, lag), limits(), **dict(params))
    return net, run_net(net), cfg


@pytest.mark.parametrize("lag", [0, 1], ids=["lag0", "lag1"])
@pytest.mark.parametrize("name,world,params,over", FLAT, ids=[case_id(*f) for f in FLAT])
def test_golden_cluster_passes_the_record(name, world, params, over, lag):
    net, outs, cfg = golden_run(name, world, params, over, lag)
    check_run(net, outs, only=GOLDEN_COUNTERS)
    check_empty(net)
    assert any(o["egress"] for o in outs)
    if lag == 0 and net.plain:
        assert_same_egress(single_oracle(net, cfg), [o["egress"] for o in outs], "single plane / cluster")


@pytest.mark.parametrize("case", sorted(SEND_CASES))
def test_golden_send_limits(case):
    """Exactly xfer_desc_max records and exactly xfer_bytes bytes pass and deliver; one
    record or 16 bytes more is refused by the model's own error."""
    cfg = dict(CFG, **SEND_CFG)
    net = SCENARIOS["send_limits"](golden_cluster(cfg, 2), limits(), case=case)
    if net.placed["fits"]:
        outs = run_net(net)
        check_run(net, outs, only=GOLDEN_COUNTERS)
        assert_same_egress(single_oracle(net, cfg), [o["egress"] for o in outs], "single plane / cluster")
    else:
        with pytest.raises(RuntimeError, match="exchange buffers too small"):
            run_net(net)


def test_limits_come_from_the_build():
    lim = limits()
    assert lim.PK_TILE == 1024 and lim.WORLD_MAX == 16 and lim.PUB_QC == 8
    # world_wide at WORLD_MAX ranks: three queues a rank, a producer and a consumer connection
    # a rank (connections 0 .. WORLD_MAX - 1 and 32 .. 32 + WORLD_MAX - 1) within the test config
    assert 32 + lim.WORLD_MAX <= CFG["c_max"] and 3 * lim.WORLD_MAX <= CFG["q_max"]


@pytest.mark.parametrize("n", [RESTORE_MAX - 1, RESTORE_MAX, RESTORE_MAX + 1, 2 * RESTORE_MAX + 1])
def test_golden_restore_keeps_item_order(n):
    """The model's restore() against the record's rendering (the device's chunking has no
    counterpart here; tests/test_gpu_xchg_edges.py compares the two)."""
    cl = golden_cluster(CFG, 1)
    dp = cl[0]
    slot = dp.declare_queue("AMQ.DEFAULT", "rq", capacity=1 << 10)
    items = restore_items(n, "rq", 1000)
    assert dp.restore([restore_tuple(it, slot) for it in items]) == n
    dp.open_connection(1, "AMQ.DEFAULT")
    dp.open_channel(1, 1)
    dp.consume(1, 1, "AMQ.DEFAULT", "rq", "rq", no_ack=True)
    eg = dp.step({}, now_ms=1)["egress"]
    assert eg[1] == b"".join(restore_wire(it, 1, t) for t, it in enumerate(items, 1))
    chunks = restore_chunks(items)
    assert sum(chunks) == n and max(chunks) <= RESTORE_MAX and len(chunks) == -(-n // RESTORE_MAX)
    big = restore_chunks(restore_items(RESTORE_MAX, "rq", 0, big=True))
    assert len(big) > 1 and max(big) < RESTORE_MAX, "the large items must cut a chunk by bytes, not by records"
    assert RESTORE_BYTES % 16 == 0
