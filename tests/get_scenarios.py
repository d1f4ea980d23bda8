"""Basic.Get between steps (``dp.basic_get``: k_basic_get on the HIP data plane) at the sizes
where the kernel changes path: its own 64-entry TTL walk and the host's GET_RETRY loop, the
GetOk / header / body renderer split at the getter's frame-max, the redelivered flag, the
channel's delivery window, the dead-letter hand-off and the ready-byte count.

Each scenario is ``(dp) -> steps`` in the ``consumer_scenarios`` style, with its own engine
overrides on top of ``gpu_cfg.CFG``.  A step may carry ``{'__get__': [(conn, channel, queue,
no_ack)]}``: the Gets are served before the step, at the step's clock; a ControlError is
recorded with its code and the queue's depth at that moment.  ``run_get`` also records, for
every step, the depth and ready bytes of every queue before and after it, a few counters, the
store records of a persisting plane and the live messages and log bytes.

``CHECKS[name]`` states what the clients must have seen, from the protocol alone: the frames
are decoded with ``chanamq_amd.protocol.codec``.  The golden model's ``basic_get`` is the
reference the HIP data plane is compared with byte by byte (tests/test_gpu_get_edges.py).

The Get buffer (``carry_cap + carry_cap / 64 + 4096`` bytes) has no golden model: its case is
stated in tests/test_gpu_get_edges.py alone.  Heads in the spill ring and in the cold store
are tests/tier_scenarios.py's."""

from collections import namedtuple

from chanamq_amd.engine.control import ControlError
from chanamq_amd.engine.traffic import ack_frame, publish_command
from chanamq_amd.protocol.codec import FrameParser, decode_method, encode_content_header
from consumer_scenarios import FM, FM_SIZES, GOLDEN_KEYS, body_of, fm_frames, nack, observe, open_ch, serial
from dp_scenarios import NOW, VH

Scenario = namedtuple("Scenario", "fn cfg now_step_ms")
STEP_MS = 2000
SHORT = {"expiration": "1000"}     # expires before the next step's clock
PERSISTENT = {"delivery_mode": 2}
PERSIST_CFG = dict(persist=1, persist_max=4096, persist_bytes=8 << 20)
DL_CFG = dict(dead_letter=True, dead_max=16, dead_bytes=1 << 20)
BYTES_CFG = dict(queue_limits=True, queue_limit_bytes=True, ucap=8)
FLAGS = ("queue_limits", "queue_limit_bytes", "dead_letter")


def a16(n):
    return (n + 15) & ~15


def slot_bytes(ex, rk, props, body):
    """A message's slot in the body log (dataplane.hip, route_one): the metadata and the body,
    each padded to 16 bytes."""
    return a16(a16(len(ex) + len(rk) + len(props)) + len(body))


# ---------------------------------------------------------------- planes and runner
def golden_plane(cfg):
    from chanamq_amd.engine.golden import GoldenDataPlane
    keys = GOLDEN_KEYS + ("ring_pool", "deliv_max", "egress_cap", "persist_max", "dead_max", "dead_bytes", "restore_max")
    kw = {k: cfg[k] for k in keys if k in cfg}
    if cfg.get("persist"):
        kw["persist"] = True
    for k in FLAGS:
        if cfg.get(k):
            kw[k] = True
    return GoldenDataPlane(**kw)


def gpu_plane(cfg, graph, **kw):
    from chanamq_amd.engine.dataplane import GpuDataPlane
    return GpuDataPlane(graph=graph, **kw, **cfg)


def is_gpu(dp):
    return hasattr(dp, "eng")


def persists(dp):
    return bool(dp.info.get("persist")) if is_gpu(dp) else bool(dp.persist)


def golden_live(g):
    """(live messages, their log slot bytes) of the golden model: what the device reports as
    n_live_msgs / live_bytes while no body is tiered."""
    msgs = {}
    for ring in g.ring.values():
        for m, _, _ in ring:
            msgs[id(m)] = m
    for st in g.ch.values():
        for sl in st["slots"].values():
            msgs[id(sl["msg"])] = sl["msg"]
    for it in g.requeue_items:
        msgs[id(it[1])] = it[1]
    for it in g.dead:
        msgs[id(it["msg"])] = it["msg"]
    live = [m for m in msgs.values() if m.refcnt > 0]
    return len(live), sum(slot_bytes(m.ex, m.rk, m.props, m.body) for m in live)


COUNTERS = ("n_deliv", "n_expired", "n_requeue", "n_dl_expired", "n_dl_pending", "n_dl_unrouted")


def serve_gets(dp, gets, now):
    out = []
    for conn, ch, qn, no_ack in gets:
        slot = dp.queues[(VH, qn)].slot
        try:
            frames, cnt = dp.basic_get(conn, ch, slot, no_ack, now_ms=now)
            out.append((frames, int(cnt)))
        except ControlError as e:
            out.append(("error", e.code, e.class_id, e.method_id, int(dp.message_count(slot))))
    return out


def queue_state(dp):
    st = dict(depth={q.name: int(dp.message_count(q.slot)) for q in dp.queues.values()})
    if getattr(dp, "queue_limit_bytes", False):
        st["bytes"] = {q.name: int(dp.queue_bytes(q.slot)) for q in dp.queues.values()}
    return st


def step_out(dp, r, gets):
    if isinstance(r, dict):
        eg, ctrl, ev, segs, tx, cnt = r["egress"], r["ctrl"], r["events"], r["segs"], r.get("txbuf", []), r["counters"]
    else:
        eg, ctrl, ev, segs, tx, cnt = r.egress, r.ctrl, r.events, [s[:4] for s in r.segs], r.txbuf, r.counters
    o = dict(egress=eg, ctrl=sorted(ctrl), events=sorted(ev), gets=gets, txbuf=sorted(tx),
             segs=sorted((s[0], s[1], s[2], s[3]) for s in segs),
             counters={c: int(cnt.get(c, 0)) for c in COUNTERS},
             qslot={q.name: q.slot for q in dp.queues.values()}, after=queue_state(dp))
    o["live"] = (int(cnt["n_live_msgs"]), int(cnt["live_bytes"])) if is_gpu(dp) else golden_live(dp)
    if persists(dp):   # store records: message ids differ between planes, the rest must not
        dp.take_persist()
        o["consumed"] = sorted((int(q), int(qpos), int(kind)) for _, q, qpos, kind in dp.take_consumed())
    return o


def run_get(dp, steps, now_step_ms=STEP_MS):
    outs = []
    for k, inp in enumerate(steps):
        inp = dict(inp)
        for op in inp.pop("__ops__", []):
            getattr(dp, op[0])(*op[1], **(op[2] if len(op) > 2 else {}))
        now = NOW + now_step_ms * k
        gets = serve_gets(dp, inp.pop("__get__", []), now)
        before = queue_state(dp)
        o = step_out(dp, dp.step(inp, now_ms=now), gets)
        o["before"] = before
        outs.append(o)
    return outs


SAME = ("counters", "after", "before", "live", "consumed")


def assert_same_get(og, od):
    """The HIP run against the golden run: ``e2e_scenarios.assert_same`` holds the wire bytes
    (the Gets' frames and counts among them), this the rest of what ``run_get`` records."""
    for k, (a, b) in enumerate(zip(og, od)):
        for f in SAME:
            assert a.get(f) == b.get(f), f"step {k} {f}: golden {a.get(f)!r}, engine {b.get(f)!r}"


# ---------------------------------------------------------------- what a Get answered
Got = namedtuple("Got", "channel tag redelivered exchange routing_key count header frames body")


def decode_get(answer):
    """One Basic.Get's answer decoded from its frames: None for GetEmpty (no frames), else the
    GetOk's fields, the raw content header and the body frames' sizes."""
    frames, _ = answer
    if frames is None:
        return None
    fr = FrameParser().feed(frames)
    assert fr[0].type == 1 and fr[1].type == 2 and all(f.type == 3 for f in fr[2:])
    assert len({f.channel for f in fr}) == 1
    m = decode_method(fr[0].payload)
    assert m.name == "basic.get_ok"
    body = b"".join(f.payload for f in fr[2:])
    assert sum(len(f.payload) + 8 for f in fr) == len(frames), "bytes between the frames"
    return Got(fr[0].channel, m.delivery_tag, bool(m.redelivered), m.exchange, m.routing_key, m.message_count,
               bytes(fr[1].payload), [len(f.payload) for f in fr[2:]], body)


def header_of(props, body):
    return encode_content_header(60, len(body), props or {})


# ---------------------------------------------------------------- the TTL walk, 64 a launch
def ttl_setup(dp, durable):
    dp.declare_queue(VH, "tq", durable=durable)
    open_ch(dp, 1)
    open_ch(dp, 2)
    return dict(PERSISTENT) if durable else {}


def ttl_pubs(lo, hi, props):
    return b"".join(publish_command(1, "", "tq", body_of("tq", i, 24), props) for i in range(lo, hi))


def sc_ttl_then_live(n, durable):
    def sc(dp):
        base = ttl_setup(dp, durable)
        return [{1: ttl_pubs(0, n, dict(base, **SHORT)) + ttl_pubs(n, n + 1, base)},
                {"__get__": [(2, 1, "tq", False)]}, {2: ack_frame(1, 1, multiple=False)}, {}]
    sc.__doc__ = f"""{n} expired entries ahead of one live entry: the host loops on GET_RETRY ({n // 64} times) and the
    Get answers the live entry with message-count 0 and tag 1."""
    return sc


def ck_ttl_then_live(n, durable):
    def ck(outs):
        (g,) = [decode_get(a) for a in outs[1]["gets"]]
        assert (g.tag, g.redelivered, g.count, g.body) == (1, False, 0, body_of("tq", n, 24))
        assert (g.exchange, g.routing_key, g.frames) == ("", "tq", [24])
        assert outs[1]["before"]["depth"] == {"tq": 0} and outs[-1]["after"]["depth"] == {"tq": 0}
        if durable:   # every skipped entry's store record (kind 1), then the Get's own (kind 3)
            q = outs[0]["qslot"]["tq"]
            assert outs[1]["consumed"] == sorted([(q, i, 1) for i in range(n)] + [(q, n, 3)])
    return ck


def sc_ttl_all_expired(n, durable):
    def sc(dp):
        base = ttl_setup(dp, durable)
        return [{1: ttl_pubs(0, n, dict(base, **SHORT))}, {"__get__": [(2, 1, "tq", False), (2, 1, "tq", True)]},
                {1: ttl_pubs(n, n + 1, base)}, {"__get__": [(2, 1, "tq", True)]}, {}]
    sc.__doc__ = f"""Exactly {n} expired entries and nothing behind them: GetEmpty with count 0 (for {n} = 64 the
    first launch cannot know, for 65 the second ends on an empty queue); a message published
    afterwards is handed out with tag 1."""
    return sc


def ck_ttl_all_expired(n, durable):
    def ck(outs):
        assert outs[1]["gets"] == [(None, 0), (None, 0)]
        assert outs[1]["before"]["depth"] == {"tq": 0}
        (g,) = [decode_get(a) for a in outs[3]["gets"]]
        assert (g.tag, g.redelivered, g.count, g.body) == (1, False, 0, body_of("tq", n, 24))
        if durable:
            q = outs[0]["qslot"]["tq"]
            assert outs[1]["consumed"] == [(q, i, 1) for i in range(n)]
            assert outs[3]["consumed"] == [(q, n, 0)]
    return ck


LIVE_FIRST = 70


def sc_ttl_live_first(durable):
    def sc(dp):
        base = ttl_setup(dp, durable)
        return [{1: ttl_pubs(0, 1, base) + ttl_pubs(1, 1 + LIVE_FIRST, dict(base, **SHORT)) + ttl_pubs(99, 100, base)},
                {"__get__": [(2, 1, "tq", True), (2, 1, "tq", True), (2, 1, "tq", True)]}, {}]
    sc.__doc__ = """A live entry at lane 0 with 70 expired ones behind it and a live one behind those: nothing is
    skipped for the first Get (count 71, the expired ones still queued), the second walks over
    the 70 (one retry), the third finds the queue empty."""
    return sc


def ck_ttl_live_first(durable):
    def ck(outs):
        a, b, c = [decode_get(x) for x in outs[1]["gets"]]
        assert (a.tag, a.count, a.body) == (1, LIVE_FIRST + 1, body_of("tq", 0, 24))
        assert (b.tag, b.count, b.body) == (2, 0, body_of("tq", 99, 24))
        assert c is None and outs[1]["gets"][2] == (None, 0)
        if durable:
            q = outs[0]["qslot"]["tq"]
            assert outs[1]["consumed"] == sorted([(q, 0, 0)] + [(q, i, 1) for i in range(1, 1 + LIVE_FIRST)]
                                                 + [(q, 1 + LIVE_FIRST, 0)])
    return ck


# ---------------------------------------------------------------- the renderer
X255 = "x" * 255
Y255 = "y" * 255
K255 = "k" * 255
BIG_PROPS = {"content_type": "application/octet-stream", "correlation_id": "c" * 100, "message_id": "m" * 100,
             "headers": {f"key-{i}": "v" * 20 for i in range(8)}, "delivery_mode": 1}
# (queue, exchange, routing key): name lengths 0 / 255 in the GetOk, which moves the header and the body
FM_ROUTES = (("fa", "", "fa"), ("fb", X255, ""), ("fc", "dx", K255), ("fd", Y255, K255))


def fm_messages():
    """[(queue, exchange, key, props, body)] in publish order: every size on every route, the
    property list alternating between none and a few hundred bytes."""
    out = []
    for r, (q, ex, rk) in enumerate(FM_ROUTES):
        for i, n in enumerate(FM_SIZES):
            out.append((q, ex, rk, BIG_PROPS if (i + r) % 2 else None, body_of(q, i, n)[:n]))
    return out


def sc_frame_split(frame_max):
    def sc(dp):
        dp.declare_exchange(VH, X255, "fanout")
        dp.declare_exchange(VH, "dx", "direct")
        dp.declare_exchange(VH, Y255, "direct")
        for q, ex, rk in FM_ROUTES:
            dp.declare_queue(VH, q)
        dp.bind(VH, "fb", X255, "")
        dp.bind(VH, "fc", "dx", K255)
        dp.bind(VH, "fd", Y255, K255)
        dp.declare_queue(VH, "fe")           # the same bodies as fb's to a consumer: deliver_size has the same split
        dp.bind(VH, "fe", X255, "")
        open_ch(dp, 1)
        open_ch(dp, 3, 2, frame_max=frame_max)
        open_ch(dp, 4, frame_max=frame_max)
        dp.consume(4, 1, VH, "fe", "e", no_ack=True)
        s = b"".join(publish_command(1, ex, rk, body, props) for q, ex, rk, props, body in fm_messages())
        gets = [(3, 2, q, True) for q, _, _ in FM_ROUTES for _ in range(len(FM_SIZES) + 1)]
        return [{1: s}, {"__get__": gets}, {}]
    sc.__doc__ = f"""Bodies of 0, 1, fm-9, fm-8, fm-7, 2(fm-8) and 2(fm-8)+1 bytes (fm = {FM}) behind exchange
    names and routing keys of 0 and 255 bytes, with and without a few hundred bytes of
    properties, handed to a getter whose connection has frame-max {frame_max}."""
    return sc


def ck_frame_split(frame_max):
    def ck(outs):
        gets = iter(outs[1]["gets"])
        tag = 0
        for q, ex, rk in FM_ROUTES:
            mine = [m for m in fm_messages() if m[0] == q]
            for i, (_, _, _, props, body) in enumerate(mine):
                g = decode_get(next(gets))
                tag += 1
                want = fm_frames(len(body)) if frame_max else ([len(body)] if body else [])
                assert (g.channel, g.tag, g.redelivered, g.exchange, g.routing_key) == (2, tag, False, ex, rk), (q, i)
                assert g.count == len(mine) - 1 - i, (q, i)
                assert g.header == header_of(props, body), (q, i)
                assert g.frames == want and g.body == body, (q, i)
                if frame_max:
                    assert all(n + 8 <= frame_max for n in g.frames) and len(g.header) + 8 <= frame_max
            assert next(gets) == (None, 0), q
        seen = [s for s in observe(outs) if s.conn == 4]
        fb = [m for m in fm_messages() if m[0] == "fb"]
        assert [(s.step, s.tag, s.body) for s in seen] == [(0, i + 1, m[4]) for i, m in enumerate(fb)]
        for s, m in zip(seen, fb):
            assert (s.frames or []) == (fm_frames(len(m[4])) if frame_max else ([len(m[4])] if m[4] else []))
    return ck


# ---------------------------------------------------------------- redelivered, window
def sc_redelivered(dp):
    """A Get with manual ack, basic.nack(requeue) of its tag, a step, then Get again: the same
    body with the flag set and the next tag; the next message has no flag."""
    dp.declare_queue(VH, "rq")
    open_ch(dp, 1)
    open_ch(dp, 2)
    s = b"".join(publish_command(1, "", "rq", body_of("rq", i, 40)) for i in range(3))
    return [{1: s}, {"__get__": [(2, 1, "rq", False)], 2: nack(1, 1, multiple=False)},
            {"__get__": [(2, 1, "rq", False)], 2: ack_frame(1, 0, multiple=True)},
            {"__get__": [(2, 1, "rq", True), (2, 1, "rq", True), (2, 1, "rq", True)]}, {}]


def ck_redelivered(outs):
    got = [decode_get(a) for o in outs for a in o["gets"]]
    assert [(g.tag, g.redelivered, serial(g.body)[1], g.count) for g in got[:4]] == [
        (1, False, 0, 2), (2, True, 0, 2), (3, False, 1, 1), (4, False, 2, 0)]
    assert got[4] is None and outs[-1]["after"]["depth"] == {"rq": 0}


UCAP = 8


def wq_pubs(n):
    return b"".join(publish_command(1, "", "wq", body_of("wq", i, 32)) for i in range(n))


def sc_window_full(dp):
    """ucap 8: eight manual-ack Gets fill the channel's window, the ninth is refused (RESOURCE_ERROR
    on 60/70) and changes nothing -- the queue still holds 4, and after an ack of tag 1 the next
    Get is tag 9 with the ninth body; the one after that is refused again."""
    dp.declare_queue(VH, "wq")
    open_ch(dp, 1)
    open_ch(dp, 2)
    return [{1: wq_pubs(12)}, {"__get__": [(2, 1, "wq", False)] * 9, 2: ack_frame(1, 1, multiple=False)},
            {"__get__": [(2, 1, "wq", False)] * 2, 2: ack_frame(1, 0, multiple=True)},
            {"__get__": [(2, 1, "wq", True)] * 4}, {}]


REFUSED = ("error", 506, 60, 70)


def ck_window_full(outs):
    a = outs[1]["gets"]
    assert [(g.tag, serial(g.body)[1], g.count) for g in map(decode_get, a[:8])] == [(i + 1, i, 11 - i) for i in range(8)]
    assert a[8] == REFUSED + (4,) and outs[1]["before"]["depth"] == {"wq": 4}
    b = outs[2]["gets"]
    g = decode_get(b[0])
    assert (g.tag, serial(g.body)[1], g.count, g.redelivered) == (9, 8, 3, False)
    assert b[1] == REFUSED + (3,)
    rest = [decode_get(x) for x in outs[3]["gets"]]
    assert [(g.tag, serial(g.body)[1]) for g in rest[:3]] == [(10, 9), (11, 10), (12, 11)] and rest[3] is None


def sc_window_noack(dp):
    """Gets with no-ack hold a window slot until the next step's window advance: the ninth in a
    row is refused like a manual-ack one, and after one step all slots are free again."""
    dp.declare_queue(VH, "wq")
    open_ch(dp, 1)
    open_ch(dp, 2)
    return [{1: wq_pubs(18)}, {"__get__": [(2, 1, "wq", True)] * 9}, {"__get__": [(2, 1, "wq", True)] * 8}, {}]


def ck_window_noack(outs):
    a = outs[1]["gets"]
    assert [(g.tag, serial(g.body)[1]) for g in map(decode_get, a[:8])] == [(i + 1, i) for i in range(8)]
    assert a[8] == REFUSED + (10,)
    b = [decode_get(x) for x in outs[2]["gets"]]
    assert [(g.tag, serial(g.body)[1]) for g in b] == [(i + 1, i) for i in range(8, 16)]
    assert outs[-1]["after"]["depth"] == {"wq": 2}


def sc_window_wrap(dp):
    """17 Gets over a window of 8 slots: slot (tag - 1) & 7 is reused twice; multiple and single
    acks in between settle the right messages -- tag 9's nack-requeue brings body 8 back (as tag 16,
    flagged), nothing else comes back, and after the last ack nothing is left."""
    dp.declare_queue(VH, "wq")
    open_ch(dp, 1)
    open_ch(dp, 2)
    get3 = [(2, 1, "wq", False)] * 3
    return [{1: wq_pubs(16)},
            {"__get__": get3, 2: ack_frame(1, 2, multiple=True)},                                       # head -> 3
            {"__get__": get3, 2: ack_frame(1, 3, multiple=False) + ack_frame(1, 4, multiple=False)},   # head -> 5
            {"__get__": get3, 2: ack_frame(1, 8, multiple=True)},                                       # head -> 9
            {"__get__": get3, 2: ack_frame(1, 10, multiple=False)},                                     # head stays
            {"__get__": get3, 2: nack(1, 9, multiple=False)},                                           # head -> 11
            {"__get__": [(2, 1, "wq", False)] * 3, 2: ack_frame(1, 0, multiple=True)}, {}]


def ck_window_wrap(outs):
    got = [decode_get(a) for o in outs for a in o["gets"]]
    assert [(g.tag, serial(g.body)[1], g.redelivered) for g in got[:17]] == (
        [(i + 1, i, False) for i in range(15)] + [(16, 8, True), (17, 15, False)])
    assert got[17] is None and len(got) == 18
    assert outs[-1]["after"]["depth"] == {"wq": 0}
    assert not any(o["egress"].get(2) for o in outs), "a Get's answer is not a delivery"


# ---------------------------------------------------------------- dead-letter queues
def dl_setup(dp):
    dp.declare_exchange(VH, "dlx", "fanout")
    dp.declare_queue(VH, "park")
    dp.bind(VH, "park", "dlx", "")
    dp.declare_queue(VH, "src", dead_letter_exchange="dlx")
    open_ch(dp, 1)
    open_ch(dp, 2)
    open_ch(dp, 3)


def src_pubs(lo, hi, props=None):
    return b"".join(publish_command(1, "", "src", body_of("src", i, 48), props) for i in range(lo, hi))


ATTACH_PARK = [("consume", (3, 1, VH, "park", "p"), dict(no_ack=True))]


def sc_dlx_heads(dp):
    """Five expired heads of a queue with a dead-letter exchange: the Get hands them to the dead
    list and answers the live entry behind them; the next step routes them, bodies intact."""
    dl_setup(dp)
    return [{1: src_pubs(0, 5, SHORT) + src_pubs(5, 6)}, {"__get__": [(2, 1, "src", True)]},
            {"__ops__": ATTACH_PARK}, {}]


def ck_dlx_heads(outs):
    (g,) = [decode_get(a) for a in outs[1]["gets"]]
    assert (g.tag, g.count, serial(g.body)[1]) == (1, 0, 5)
    seen = [s for s in observe(outs) if s.conn == 3]
    assert [s.body for s in seen] == [body_of("src", i, 48) for i in range(5)]
    assert outs[-1]["after"]["depth"] == {"park": 0, "src": 0}


DL_N = 20


def sc_dlx_list_full(dp):
    """A dead list of 16 and 20 expired heads: the Get fills the list, answers GetEmpty with the
    count of what is still queued (4 expired and the live one), and after a step drained the
    list a Get continues and answers the live entry.  All 20 dead letters arrive, in order."""
    dl_setup(dp)
    return [{1: src_pubs(0, DL_N, SHORT) + src_pubs(DL_N, DL_N + 1)}, {"__get__": [(2, 1, "src", True)]},
            {"__get__": [(2, 1, "src", True)], "__ops__": ATTACH_PARK}, {}, {}]


def ck_dlx_list_full(outs):
    assert outs[1]["gets"] == [(None, DL_N + 1 - DL_CFG["dead_max"])]
    assert outs[1]["before"]["depth"]["src"] == DL_N + 1 - DL_CFG["dead_max"]
    (g,) = [decode_get(a) for a in outs[2]["gets"]]
    assert (g.tag, g.count, serial(g.body)[1]) == (1, 0, DL_N)
    seen = [s for s in observe(outs) if s.conn == 3]
    assert [s.body for s in seen] == [body_of("src", i, 48) for i in range(DL_N)]
    assert outs[-1]["after"]["depth"] == {"park": 0, "src": 0}


# ---------------------------------------------------------------- ready bytes
BQ = dict(ok=((100, 200, 300), (400, 500)), win=((64, 65), (700, 20)), empty=((33, 34, 35), ()))   # (expired, live) sizes


def sc_bytes_exits(dp):
    """queue_limit_bytes on: the ready bytes after a Get that skipped expired entries and took
    one, and after the exits that take nothing -- the window full (the skip still happened) and
    an empty queue."""
    for q in BQ:
        dp.declare_queue(VH, q, max_length_bytes=1 << 20)
    dp.declare_queue(VH, "fill")
    open_ch(dp, 1)
    open_ch(dp, 2)
    s = b""
    for q, (dead, live) in BQ.items():
        s += b"".join(publish_command(1, "", q, body_of(q, i, n), SHORT) for i, n in enumerate(dead))
        s += b"".join(publish_command(1, "", q, body_of(q, 10 + i, n)) for i, n in enumerate(live))
    s += b"".join(publish_command(1, "", "fill", body_of("fill", i, 16)) for i in range(UCAP - 1))
    gets = [(2, 1, "ok", False), (2, 1, "empty", False)] + [(2, 1, "fill", False)] * (UCAP - 1) + [(2, 1, "win", False)]
    drain = [(2, 1, "ok", True), (2, 1, "win", True), (2, 1, "win", True)]
    return [{1: s}, {"__get__": gets, 2: ack_frame(1, 0, multiple=True)}, {"__get__": drain}, {}]


def ck_bytes_exits(outs):
    total = {q: sum(dead) + sum(live) for q, (dead, live) in BQ.items()}
    assert outs[0]["after"]["bytes"] == dict(total, fill=16 * (UCAP - 1))
    a = outs[1]["gets"]
    g = decode_get(a[0])
    assert (g.tag, len(g.body), g.count) == (1, 400, 1)
    assert a[1] == (None, 0) and a[-1] == REFUSED + (2,)
    assert outs[1]["before"]["bytes"] == dict(ok=500, win=720, empty=0, fill=0)
    assert outs[1]["before"]["depth"] == dict(ok=1, win=2, empty=0, fill=0)
    assert [len(decode_get(x).body) for x in outs[2]["gets"]] == [500, 700, 20]
    assert outs[2]["before"]["bytes"] == dict(ok=0, win=0, empty=0, fill=0)


# ---------------------------------------------------------------- the tables
SCENARIOS, CHECKS = {}, {}


def _add(name, fn, ck, cfg=None, now_step_ms=STEP_MS):
    SCENARIOS[name] = Scenario(fn, cfg or {}, now_step_ms)
    CHECKS[name] = ck


for _dur, _sfx, _cfg in ((False, "", {}), (True, "_durable", PERSIST_CFG)):
    for _n in (63, 64, 65, 128, 129):
        _add(f"ttl_{_n}_then_live{_sfx}", sc_ttl_then_live(_n, _dur), ck_ttl_then_live(_n, _dur), _cfg)
    for _n in (64, 65):
        _add(f"ttl_{_n}_all_expired{_sfx}", sc_ttl_all_expired(_n, _dur), ck_ttl_all_expired(_n, _dur), _cfg)
    _add(f"ttl_live_first{_sfx}", sc_ttl_live_first(_dur), ck_ttl_live_first(_dur), _cfg)
_add("frame_split_fm4096", sc_frame_split(FM), ck_frame_split(FM))
_add("frame_split_fm0", sc_frame_split(0), ck_frame_split(0))
_add("redelivered", sc_redelivered, ck_redelivered)
_add("window_full", sc_window_full, ck_window_full, dict(ucap=UCAP))
_add("window_noack", sc_window_noack, ck_window_noack, dict(ucap=UCAP))
_add("window_wrap", sc_window_wrap, ck_window_wrap, dict(ucap=UCAP))
_add("dlx_heads", sc_dlx_heads, ck_dlx_heads, DL_CFG)
_add("dlx_list_full", sc_dlx_list_full, ck_dlx_list_full, DL_CFG)
_add("bytes_exits", sc_bytes_exits, ck_bytes_exits, BYTES_CFG)
