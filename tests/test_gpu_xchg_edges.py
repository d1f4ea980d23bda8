"""The sharded half of the HIP data plane -- k_pack_scan, k_pack / pack_one, k_import_route /
import_one and the host-injected import path behind ``Engine::restore`` -- at the places where
those kernels change path: every scenario of tests/xchg_scenarios.py on a ``LocalCluster`` of
``GpuDataPlane`` on one device, in the captured graph and with eager launches, without a lag
and with ``exchange_lag`` 1.  A run is judged by the scenario's own record (every connection's
egress rendered by the host codec; what phase A packed against the record's serialiser, before
the exchange moves it; the device's per-publish remote masks), then compared byte for byte
with the golden cluster and, without a lag, with one golden plane holding every connection.
The capacity exits (send buffers, import buffers, restore chunks) run at their limit and one
past it; the checks that refuse a bad host-injected record run without touching the device."""

import time

import numpy as np
import pytest

from chanamq_amd.engine.layout import MF_HOSTPUB, MF_PERSIST, RDESC
from chanamq_amd.parallel.cluster import _gpu_submit
from chanamq_amd.protocol.codec import Method, encode_properties, render_command
from egress_scenarios import body_of, command
from gpu_cfg import CFG
from test_golden_xchg_edges import CASES, case_id
from xchg_scenarios import (BOTH, PERSISTENT, RECV_CFG, RECV_MAX, RESTORE_BYTES, RESTORE_MAX, SCENARIOS,
                            SEND_CASES, SEND_CFG, VH, Net, assert_same_egress, check_empty, check_run, cluster_step,
                            golden_cluster, gpu_cluster, limits, restore_chunks, restore_items, restore_tuple,
                            restore_wire, run_net, single_oracle)

pytestmark = pytest.mark.gpu

MODES = {"graph": True, "eager": False}
ALL = [("graph", 0), ("graph", 1), ("eager", 0), ("eager", 1)]
SOME = [("graph", 0), ("eager", 1)]
RUNS = [(n, w, tuple(sorted(p.items())), tuple(sorted(c.items())), mode, lag)
        for n, cs in CASES.items() for w, p, c in cs
        for mode, lag in (ALL if n in ("step_sequence", "record_fields") else SOME)]
_golden = {}


def golden_outs(name, world, params, over, lag):
    """The golden cluster's run of a case and, without a lag, the single plane's: computed
    once, only read by the cases."""
    key = (name, world, params, over, lag)
    if key not in _golden:
        cfg = dict(CFG, **dict(over))
        net = SCENARIOS[name](golden_cluster(cfg, world, lag), limits(), **dict(params))
        outs = [o["egress"] for o in run_net(net)]
        _golden[key] = (outs, single_oracle(net, cfg) if lag == 0 and net.plain else None)
    return _golden[key]


def check_build(cl, lim):
    for p in cl.planes:
        assert p.info["pk_tile"] == lim.PK_TILE and p.info["world_max"] == lim.WORLD_MAX


@pytest.mark.parametrize("name,world,params,over,mode,lag", RUNS, ids=[case_id(*r[:5]) + f"-lag{r[5]}" for r in RUNS])
def test_xchg_edges(gpu, name, world, params, over, mode, lag):
    lim = limits()
    cfg = dict(CFG, **dict(over))
    cl = gpu_cluster(cfg, world, lag, MODES[mode])
    check_build(cl, lim)
    net = SCENARIOS[name](cl, lim, **dict(params))
    assert net.lag == lag
    outs = run_net(net)
    check_run(net, outs)                       # the record: egress, send counts, counters; send buffers in run_net
    check_empty(net)
    want, single = golden_outs(name, world, params, over, lag)
    assert_same_egress(want, [o["egress"] for o in outs], "golden cluster / device")
    if single is not None:
        assert_same_egress(single, [o["egress"] for o in outs], "single plane / device")
    info = cl[0].info
    if name == "tile_edges":     # the steps sit on the tile edges of this build, the last one fills the step
        assert info["pub_max"] == 4 * lim.PK_TILE and net.placed["tiles"] == [1, 1, 1, 1, 1, 1, 2, 3, 4]
        assert net.pack == set(range(12))
    elif name == "many_tiles":   # more tiles than one round of the prefix loop takes
        assert info["pub_max"] >= 65 * lim.PK_TILE + 1 and net.placed["tiles"] == 66 > 64
        assert outs[0]["counters"][0]["n_pubs"] == 65 * lim.PK_TILE + 1 and outs[0]["sent"][0][1] == 16
    elif name == "world_wide":
        assert world in (8, lim.WORLD_MAX) and info["world"] == world
        # pair key = queue bits + the one source bit: one fused pass of 8 bits (q_max 64) and of 11
        # (q_max 512), and at q_max 1024 two 8-bit passes, k_qfirst, k_ring_plan and k_enqueue
        bits = net.placed["key_bits"]
        assert bits == {64: 8, 512: lim.SORT_ONEPASS_BITS, 1024: lim.SORT_ONEPASS_BITS + 1}[cfg["q_max"]]
        if cfg["q_max"] > 64:   # the key's top queue bit is in use
            assert max(net.placed["slots"]) == cfg["q_max"] - 1
        assert all(sum(o[:world]) > 0 and all(n > 0 for d, n in enumerate(o[:world]) if d != r)
                   for r, o in enumerate(outs[0]["sent"]))
    elif name == "oneq_paths":
        assert net.placed["oneq"] > 0 and net.placed["rematched"] > 0
    elif name == "step_sequence":
        assert [o["sent"][0][1] for o in outs[:5]] == net.placed["sent"] == [0, lim.PK_TILE + 1, 0, 1, 0]
    elif name == "recv_limits":
        assert cl[2].info["import_max"] == RECV_MAX == net.placed["received"]


# ---------------------------------------------------------------- the send buffers at their limit
@pytest.mark.parametrize("case", sorted(SEND_CASES))
def test_send_limits(gpu, case):
    """xfer_desc_max records and xfer_bytes bytes exactly pass and deliver everything; one
    record or 16 bytes more raises the overflow error from submit_raw, and the rank finishes
    the step with nothing received.  pack_one skips a record whose descriptor index or whose
    last payload byte lies past its buffer, so neither case stores outside one."""
    lim = limits()
    cfg = dict(CFG, **SEND_CFG)
    cl = gpu_cluster(cfg, 2)
    assert cl[0].info["xfer_desc_max"] == SEND_CFG["xfer_desc_max"] and cl[0].info["xfer_bytes"] == SEND_CFG["xfer_bytes"]
    net = SCENARIOS["send_limits"](cl, lim, case=case)
    if net.placed["fits"]:
        outs = run_net(net)
        check_run(net, outs)
        g = SCENARIOS["send_limits"](golden_cluster(cfg, 2), lim, case=case)
        assert_same_egress([o["egress"] for o in run_net(g)], [o["egress"] for o in outs], "golden cluster / device")
        assert sum(outs[0]["sent"][0][2:]) == net.placed["bytes"]
        return
    with pytest.raises(RuntimeError, match="send buffers overflowed"):
        run_net(net)
    # Phase A is through; the step ends as one that received nothing.  submit_raw raised before it
    # returned its ticket, so the ticket is put together here as GpuDataPlane.submit_raw does:
    # (parity, segments, start time, egress slot), the parity being the one it left in _pending.
    d = cl[0]
    par = d._pending
    d.submit_b([0, 0, 0, 0])
    res = d.finish((par, 1, time.perf_counter(), d.eng.egress_slot(par)))
    assert not res.egress and res.counters["n_pubs"] == net.placed["records"]
    assert cl[1].message_count(net.slot["qs"]) == 0


# ---------------------------------------------------------------- the import buffers past their limit
@pytest.mark.parametrize("mode", sorted(MODES))
def test_recv_over_limit_is_dropped_whole(gpu, mode):
    """Counts one above import_max handed to phase B with nothing copied: nothing is imported,
    n_dropped_nomem rises by the count, and the next step is a normal one."""
    lim = limits()
    cl = gpu_cluster(dict(CFG, **RECV_CFG), 3, 0, MODES[mode])
    net = SCENARIOS["recv_limits"](cl, lim)
    seen = {}

    def over():
        k = net.placed["normal_again"]
        tickets = [_gpu_submit(p, {}, net.now(k)) for p in cl.planes]
        assert all(sum(p.pending_send_counts()) == 0 for p in cl.planes)
        recv = [[0] * 6, [0] * 6, [RECV_MAX // 2 + 1, RECV_MAX // 2, 0, 0, 0, 0]]
        for r, p in enumerate(cl.planes):
            p.submit_b(recv[r])
        seen["res"] = [p.finish(t) for p, t in zip(cl.planes, tickets)]
    net.ops[net.placed["normal_again"]].append(over)
    outs = run_net(net)
    res = seen["res"]
    assert res[2].counters["n_dropped_nomem"] == RECV_MAX + 1 and res[2].counters["n_deliv"] == 0
    assert all(not r.egress for r in res) and res[0].counters["n_dropped_nomem"] == 0
    check_run(net, outs)           # the steps before it, and the normal step after it
    check_empty(net)
    assert outs[net.placed["normal_again"]]["counters"][2]["n_dropped_nomem"] == 0


# ---------------------------------------------------------------- restore, publish_host, publish_to_queues
PERSIST = dict(persist=1, persist_max=4096, persist_bytes=8 << 20, restore_max=RESTORE_MAX)


def restore_cluster(world, **kw):
    size = {"restore_bytes": RESTORE_BYTES} if world == 1 else {"xfer_bytes": RESTORE_BYTES}
    cl = gpu_cluster(dict(CFG, **PERSIST, **size), world, **kw)
    assert cl[0].info["restore_max"] == RESTORE_MAX and cl[0].info["xfer_bytes"] == RESTORE_BYTES
    return cl


class CountingEngine:
    """The plane's engine with its restore() calls noted: (records, payload bytes) of each."""

    def __init__(self, eng):
        self._eng, self.restores = eng, []

    def __getattr__(self, name):
        return getattr(self._eng, name)

    def restore(self, desc, pay, now):
        self.restores.append((desc.nbytes // RDESC.itemsize, pay.nbytes))
        return self._eng.restore(desc, pay, now)


def drain_queue(cl, net, q, now):
    """Attach the queue's consumer and step until it is empty -> (its connection's egress,
    the consumed records of those steps)."""
    net.consume(q)
    conn = net.cons[q][0]
    eg, recs = b"", []
    for k in range(8):
        res = cluster_step(cl, [{} for _ in cl.planes], now + k)
        eg += res[net.owner[q]][0].get(conn, b"")
        recs += cl[net.owner[q]].take_consumed()
        if not cl[net.owner[q]].message_count(net.slot[q]):
            break
    return eg, recs


@pytest.mark.parametrize("world", [1, 2])
def test_restore_edges(gpu, world):
    """restore() of restore_max - 1 .. 2 * restore_max + 1 items and of items whose bytes pass
    the payload buffer inside a chunk (records in the host layout: the body follows the
    properties, write_slot stores them): every item lands in its queue in item order across
    the chunk edges, with its redelivered flag and its own message id; an item for a queue of
    another rank is not stored."""
    cl = restore_cluster(world)
    net = Net(cl, limits())
    dp = cl[0]
    ns = (RESTORE_MAX - 1, RESTORE_MAX, RESTORE_MAX + 1, 2 * RESTORE_MAX + 1)
    for i in range(len(ns) + 1):
        net.queue(f"rq{i}", 0, capacity=1 << 10, consume=False, durable=True)
    if world > 1:
        net.queue("away", 1, capacity=1 << 10, consume=False, durable=True)
    batches = [restore_items(n, f"rq{i}", 1000 * (i + 1)) for i, n in enumerate(ns)]
    batches.append(restore_items(RESTORE_MAX, f"rq{len(ns)}", 9000, big=True))
    assert [len(restore_chunks(b)) for b in batches[:4]] == [1, 1, 2, 3] and len(restore_chunks(batches[4])) > 2
    dp.eng = counted = CountingEngine(dp.eng)
    for i, items in enumerate(batches):
        sent = list(items)
        if world > 1 and i == 2:    # some for the other rank's queue, in between
            sent[5:5] = restore_items(3, "away", 77)
        del counted.restores[:]
        assert dp.restore([restore_tuple(it, net.slot[it.queue]) for it in sent], now_ms=1000) == len(items)
        # the batches the engine was handed: every item once, each batch within the buffers, and
        # as many as the record cuts by records (by bytes restore() may cut sooner, never later)
        calls = counted.restores
        assert sum(n for n, _ in calls) == len(sent) and all(n <= RESTORE_MAX and b <= RESTORE_BYTES for n, b in calls)
        assert len(calls) >= len(restore_chunks(sent)) and (i == 4 or len(calls) == len(restore_chunks(sent))), (i, calls)
        assert i != 4 or max(n for n, _ in calls) < RESTORE_MAX, "the large items cut a batch by bytes"
        assert dp.message_count(net.slot[f"rq{i}"]) == len(items)
    dp.eng = counted._eng
    if world > 1:
        assert cl[0].message_count(net.slot["away"]) == 0 and cl[1].message_count(net.slot["away"]) == 0
    for i, items in enumerate(batches):
        eg, recs = drain_queue(cl, net, f"rq{i}", 2000 + 10 * i)
        ch = net.cons[f"rq{i}"][1]
        assert eg == b"".join(restore_wire(it, ch, t) for t, it in enumerate(items, 1)), f"batch {i}"
        kept = sorted((qpos, mid) for mid, q, qpos, kind in recs if q == net.slot[f"rq{i}"])
        assert kept == [(pos, it.mid) for pos, it in enumerate(items) if it.persistent], f"batch {i}: message ids"


def test_restore_is_refused_under_a_lagged_exchange(gpu):
    """Rank 1 publishes for a queue of rank 0; after that step the records wait in rank 0's
    receive buffer for the next step's phase B.  restore() on rank 0, which would write its
    batch over them, is refused, and the next step delivers them."""
    cl = restore_cluster(2, lag=1)
    net = Net(cl, limits())
    net.exchange("lx", "fanout")
    net.queue("lq", 0), net.bind("lq", "lx")
    net.queue("rq", 0, consume=False)
    net.open(1, 1)
    for i in range(5):
        net.pub(1, "lx", "k", 30 + i, PERSISTENT)
    net.step(sent={1: [5, 0]})
    tried = []

    def refused():
        items = restore_items(2, "rq", 1)
        with pytest.raises(RuntimeError, match="lagged exchange"):
            cl[0].restore([restore_tuple(it, net.slot["rq"]) for it in items], now_ms=1)
        assert cl[0].message_count(net.slot["rq"]) == 0
        tried.append(1)
    net.ops[1].append(refused)
    net.drain()
    outs = run_net(net)
    assert tried and not outs[0]["egress"] and outs[1]["egress"]
    check_run(net, outs)
    check_empty(net)


def test_host_records_out_of_range_are_refused(gpu):
    """import_one indexes q_owner with a routed record's queue slot and ch_pub_fail with a host
    publish's channel slot as given: Engine::restore refuses what lies outside the tables, and
    a payload offset past the payload, before anything reaches the device."""
    cl = restore_cluster(1)
    dp = cl[0]
    q_max, nch = dp.info["q_max"], dp.info["c_max"] * dp.info["chpc"]
    with pytest.raises(RuntimeError, match="queue slot"):
        dp.publish_to_queues([q_max], b"x", b"k", encode_properties({}), b"body", 0, now_ms=1)
    with pytest.raises(RuntimeError, match="queue slot"):
        dp.restore([(q_max + 7, 1, 0, 0, b"x", b"k", encode_properties({}), b"body", False, False)], now_ms=1)
    desc = np.zeros(1, RDESC)
    desc[0]["flags"], desc[0]["body_len"] = MF_HOSTPUB, 16
    pay = np.zeros(16, np.uint8)
    for pad in ((nch, 0), (0, dp.info["c_max"])):
        desc[0]["pad"][0], desc[0]["pad"][1] = pad
        with pytest.raises(RuntimeError, match="channel out of range"):
            dp.eng.restore(desc.view(np.uint8), pay, 1)
    desc[0]["pad"][:2] = 0
    desc[0]["exch"] = dp.info["x_max"]
    with pytest.raises(RuntimeError, match="exchange slot"):
        dp.eng.restore(desc.view(np.uint8), pay, 1)
    desc[0]["exch"] = -1
    with pytest.raises(RuntimeError, match="no whole records"):
        dp.eng.restore(desc.view(np.uint8)[:40], pay, 1)
    desc[0]["pay_off"] = 16
    with pytest.raises(RuntimeError, match="past its payload"):
        dp.eng.restore(desc.view(np.uint8), pay, 1)
    r = dp.step({}, now_ms=2)
    assert not r.egress and r.counters["n_routed_msgs"] == 0


@pytest.mark.parametrize("world", [1, 2])
def test_publish_host_and_publish_to_queues(gpu, world):
    """publish_host: routed by its exchange, counted for the channel's confirm, 0 for an
    unroutable one, stored in this rank's queues only.  publish_to_queues to 1, PUB_QC and
    PUB_QC + 1 queues: one message each, every one with an id of its own."""
    lim = limits()
    cl = restore_cluster(world)
    net = Net(cl, lim)
    dp = cl[0]
    net.exchange("hx", "direct")
    net.queue("h0", 0, consume=False), net.bind("h0", "hx", "both")
    net.queue("h1", world - 1, consume=False), net.bind("h1", "hx", "both")
    sizes = (1, lim.PUB_QC, lim.PUB_QC + 1)
    for n in sizes:
        for i in range(n):
            net.queue(f"t{n}_{i}", 0, consume=False, durable=True)
    net.open(1, 0, confirm=True)
    props, body = encode_properties(BOTH), body_of(1, 300)
    x = dp.exchanges[(VH, "hx")].slot
    assert dp.publish_host(1, 1, x, b"hx", b"both", props, body, MF_PERSIST, ts_ms=BOTH["timestamp"] * 1000, now_ms=10) == 1
    assert dp.publish_host(1, 1, x, b"hx", b"nobody", props, body, 0, now_ms=11) == 0
    assert dp.message_count(net.slot["h0"]) == 1
    assert cl[world - 1].message_count(net.slot["h1"]) == (0 if world > 1 else 1)
    net.consume("h0")
    res = cluster_step(cl, [{} for _ in cl.planes], 12)
    conn, ch, _ = net.cons["h0"]
    m = Method("basic.deliver", consumer_tag="h0", delivery_tag=1, redelivered=False, exchange="hx", routing_key="both")
    assert res[0][0].get(conn) == command(ch, m, BOTH, body)
    assert res[0][0].get(1) == render_command(1, Method("basic.ack", delivery_tag=2, multiple=True))
    ids = []
    for n in sizes:
        slots = [net.slot[f"t{n}_{i}"] for i in range(n)]
        assert dp.publish_to_queues(slots, b"px", b"key", encode_properties(PERSISTENT), body_of(n, 40 + n), MF_PERSIST,
                                    now_ms=20) == n
        assert [dp.message_count(s) for s in slots] == [1] * n
        for i in range(n):
            eg, recs = drain_queue(cl, net, f"t{n}_{i}", 30)
            m = Method("basic.deliver", consumer_tag=f"t{n}_{i}", delivery_tag=1, redelivered=False, exchange="px",
                       routing_key="key")
            assert eg == command(net.cons[f"t{n}_{i}"][1], m, PERSISTENT, body_of(n, 40 + n))
            ids += [mid for mid, q, qpos, kind in recs if q == slots[i]]
    assert len(ids) == sum(sizes) == len(set(ids)), "every queue's copy has a message id of its own"
