"""Priority queues on the HIP data plane: k_prio_lane, k_prio_dispatch and the PRIO instantiations
of k_dequeue and k_dead_pack (csrc/kernels/dp_prio.h, dataplane.hip).  Every scenario of
tests/prio_scenarios.py, in the captured graph and with eager launches, at the default q_max and
at q_max = 4096 (the two pair-key widths, so both sort paths), judged by the scenarios' own record
and then compared step by step with the golden model: egress bytes, counters, depths per lane and
ring capacities must be equal."""

import pytest
import torch  # noqa: F401  (loaded before the extension initialises HIP)

from gpu_cfg import CFG
from prio_scenarios import DEVICE_ONLY, OFF, SCENARIOS, WIDTHS, cfg_of, check, compare, golden_plane, gpu_plane, run_prio
from dp_scenarios import NOW, VH
from route_scenarios import check_drained

pytestmark = pytest.mark.gpu

MODES = {"graph": True, "eager": False}
_golden = {}


def golden_outs(sc, key, cfg, on=True):
    """The golden model's run of a scenario: computed once, only read by the cases."""
    if key not in _golden:
        g = golden_plane(cfg, on)
        _golden[key] = run_prio(g, sc.fn(g, on))
    return _golden[key]


def judge(sc, key, mode, width, on=True):
    cfg = dict(cfg_of(sc, CFG), **WIDTHS[width])
    d = gpu_plane(cfg, MODES[mode], on)
    assert d.info["priority_queues"] == int(on)
    rec = sc.fn(d, on)
    od = run_prio(d, rec)
    check(rec, od)
    compare(golden_outs(sc, (key, width), cfg, on), od)
    if sc.drained:
        check_drained(d.last_counters, cfg["log_block"])
        assert all(d.message_count(q.slot) == 0 for q in d.queues.values())
    return d


@pytest.mark.parametrize("width", sorted(WIDTHS))
@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_prio(gpu, name, mode, width):
    judge(SCENARIOS[name], name, mode, width)


@pytest.mark.parametrize("width", sorted(WIDTHS))
@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("name", sorted(DEVICE_ONLY))
def test_step_cuts(gpu, name, mode, width):
    """The egress budget and deliv_max ending inside a lane, and a publish the full pair table cuts
    short (on both sort paths): the golden model has none of the three bounds, so the scenarios' own
    record, which has the rules written into it, is the judge."""
    sc = DEVICE_ONLY[name]
    cfg = dict(cfg_of(sc, CFG), **WIDTHS[width])
    d = gpu_plane(cfg, MODES[mode])
    assert all(d.info[k] == v for k, v in sc.cfg.items())
    rec = sc.fn(d)
    od = run_prio(d, rec)
    check(rec, od)
    assert any(w["counters"]["n_deliv"] for w in rec.want)
    check_drained(d.last_counters, cfg["log_block"])
    assert all(d.message_count(q.slot) == 0 for q in d.queues.values())


@pytest.mark.parametrize("mode", sorted(MODES))
def test_off_is_today(gpu, mode):
    """The flag off: x-max-priority is ignored, ``info`` reports 0 and the queue is a FIFO."""
    d = judge(OFF, "off", mode, "narrow", on=False)
    assert len(d.queue_by_slot) == 1


def test_basic_get_between_steps(gpu):
    """GpuDataPlane.basic_get on a priority queue: the highest lane that holds a message, the count
    over all lanes, GetEmpty on an empty queue -- equal to the golden model's answers."""
    from chanamq_amd.engine.traffic import publish_command
    answers = []
    for dp in (golden_plane(CFG), gpu_plane(CFG, True)):
        s = dp.declare_queue(VH, "bg", max_priority=3)
        dp.open_connection(1, VH)
        dp.open_channel(1, 1)
        dp.open_connection(2, VH)
        dp.open_channel(2, 1)
        got = [dp.basic_get(2, 1, s, True, NOW)]
        dp.step({1: b"".join(publish_command(1, "", "bg", b"m%d" % i, {"priority": p} if p is not None else None)
                             for i, p in enumerate([0, 2, None, 2, 1]))}, now_ms=NOW)
        for _ in range(6):
            got.append(dp.basic_get(2, 1, s, True, NOW))
        answers.append(got)
        assert [c for _, c in got] == [0, 4, 3, 2, 1, 0, 0]
        assert [f is not None and f[f.index(b"m"):f.index(b"m") + 2] for f, _ in got[1:6]] == [b"m1", b"m3", b"m4", b"m0", b"m2"]
        assert got[0][0] is None and got[6][0] is None
    assert answers[0] == answers[1]


def deliveries(raw):
    """[(method name, body, message-count or None)] of one connection's egress."""
    from chanamq_amd.protocol.codec import CommandAssembler, FrameParser
    fp, ca = FrameParser(), CommandAssembler()
    out = []
    for f in fp.feed(raw):
        c = ca.feed(f)
        if c is not None:
            out.append((c.method.name, bytes(c.body or b""), getattr(c.method, "message_count", None)))
    return out


@pytest.mark.parametrize("mode", sorted(MODES))
def test_host_staged_and_decoded_gets_in_one_step(gpu, mode):
    """Gets the host staged for the step (the pipelined front end's path: GetReq / GetOut) and Gets
    decoded from a connection's bytes, for one priority queue in one step: the staged ones are
    served first, in request order, then the decoded ones, all from the front of V with the count
    over all lanes; a staged Get of an empty priority queue is answered EMPTY."""
    import numpy as np
    from chanamq_amd.engine.traffic import publish_command
    from dp_scenarios import get_cmd
    d = gpu_plane(CFG, MODES[mode])
    s = d.declare_queue(VH, "hg", max_priority=2)
    e = d.declare_queue(VH, "he", max_priority=1)
    for conn in (1, 2, 3):
        d.open_connection(conn, VH)
        d.open_channel(conn, 1)
    d.step({1: b"".join(publish_command(1, "", "hg", b"m%d" % i, {"priority": p}) for i, p in enumerate([0, 2, 1, 0, 1]))},
           now_ms=NOW)
    d.eng.stage_gets(np.array([[3, d.chslot(3, 1), s, 1], [3, d.chslot(3, 1), e, 1], [3, d.chslot(3, 1), s, 1]], np.uint32))
    r = d.step({2: get_cmd(1, "hg", True) * 2}, now_ms=NOW)
    assert [tuple(x) for x in d.eng.get_out(d._last_parity)] == [(1, 4), (0, 0), (1, 3)]      # GS_OK, GS_EMPTY, GS_OK
    assert deliveries(r.egress[3]) == [("basic.get_ok", b"m1", 4), ("basic.get_ok", b"m2", 3)]
    assert deliveries(r.egress[2]) == [("basic.get_ok", b"m4", 2), ("basic.get_ok", b"m0", 1)]
    assert [int(d._u64("q_tail", s + k) - d._u64("q_head", s + k)) for k in range(3)] == [0, 0, 1]
    assert d.message_count(s) == 1


def test_host_assembled_publish_lands_on_its_lane(gpu):
    """publish_host (a message the host assembled, imported from the restore buffer between
    steps) and publish_to_queues into a priority queue: k_prio_lane reads their property bytes
    from that buffer."""
    from chanamq_amd.protocol.codec import encode_properties
    d = gpu_plane(CFG, True)
    s = d.declare_queue(VH, "hp", max_priority=3)
    d.open_connection(1, VH)
    d.open_channel(1, 1)
    d.open_connection(2, VH)
    d.open_channel(2, 1)
    xs = d.exchanges[(VH, "")].slot
    for i, p in enumerate([1, 3, None, 2, 9]):
        props = encode_properties({"priority": p, "content_type": "t"} if p is not None else {"content_type": "t"})
        d.publish_host(1, 1, xs, b"", b"hp", props, b"h%d" % i, 0, now_ms=NOW)
    d.publish_to_queues([s], b"", b"hp", encode_properties({"priority": 2}), b"q5", 0, now_ms=NOW)
    assert [int(d._u64("q_tail", s + k) - d._u64("q_head", s + k)) for k in range(4)] == [2, 2, 1, 1]
    d.consume(2, 1, VH, "hp", "c", no_ack=True)
    r = d.step({}, now_ms=NOW)
    assert [b for _, b, _ in deliveries(r.egress[2])] == [b"h1", b"h4", b"h3", b"q5", b"h0", b"h2"]


def test_cold_store_takes_no_lane_body(gpu):
    """What the cold pick lists in the slots of a priority queue is left out before anything is
    stored or committed; an ordinary queue's records pass."""
    import numpy as np
    from chanamq_amd.store.cold import COLD_REC
    d = gpu_plane(CFG, True)
    s = d.declare_queue(VH, "cp", max_priority=2)
    plain = d.declare_queue(VH, "co")

    class Store:
        def put_many(self, views):
            raise AssertionError("a lane body reached the store")

    recs = np.zeros(3, COLD_REC)
    recs["q"], recs["bytes"] = [s, s + 1, s + 2], 64
    assert d._cold_store(Store(), recs) is None
    assert plain == s + 3 and d.lane_slots(plain) == [plain]
