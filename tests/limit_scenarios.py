"""Queue length limits (x-max-length / x-overflow, ``queue_limits=True``) in the
``consumer_scenarios`` style: each scenario is ``(dp, on) -> Rec`` with its own engine
overrides on top of ``gpu_cfg.CFG``.

``Rec`` is the scenarios' own record: a plain Python list per queue, to which it applies the
rules of the feature as they are written down -- reject-publish refuses at enqueue what would
exceed the limit (requeues are never refused), drop-head trims the head at the end of the
queue's step, after its enqueue, requeues, TTL walk, Basic.Gets and dispatch.  While a
scenario is written, the record builds the wire input of every step and predicts what the
step must put on the wire (every delivery and GetOk in order, every GetEmpty, every Basic.Ack
and Basic.Nack), the queue depths it leaves and the step's counters.  It never looks at the
golden model: ``check`` judges the golden model's run and the HIP data plane's alike.
"""

from collections import defaultdict, namedtuple

from chanamq_amd.engine.traffic import ack_frame, publish_command
from chanamq_amd.protocol.codec import FrameParser, decode_content_header, decode_method
from consumer_scenarios import GOLDEN_KEYS, body_of, nack
from dp_scenarios import NOW, VH, get_cmd

Scenario = namedtuple("Scenario", "fn cfg now_step_ms drained")
COUNTERS = ("n_deliv", "n_expired", "n_requeue", "n_ring_full", "n_maxlen_dropped", "n_maxlen_rejected")
DELIVER_CAP = 4096     # gpu_cfg.CFG deliver_cap: one consumer's deliveries per step
PERSISTENT = {"delivery_mode": 2}


class Entry:
    __slots__ = ("body", "expire", "red", "seq")

    def __init__(self, body, expire, seq):
        self.body, self.expire, self.red, self.seq = body, expire, False, seq


class Rec:
    """The record.  Topology calls go to the plane at once; traffic calls (``pub``, ``ack_all``,
    ``nack_all``, ``get``, ``op``) collect the current step, ``end`` closes it: the step's wire
    input goes to ``steps`` and what it must lead to goes to ``want``."""

    def __init__(self, dp, on=True, now_step_ms=0, ucap=256):
        self.dp, self.on, self.now_step_ms, self.ucap = dp, on, now_step_ms, ucap
        self.q = {}                       # name -> dict(slot, L, mode, ttl, durable, items, cons, serial)
        self.chan = {}                    # (conn, ch) -> dict(confirm, pubs, tag, unacked, flow, win)
        self.fan = defaultdict(list)      # fanout exchange -> [queue]
        self.steps, self.want = [], []
        self.seq = 0
        self._new_step()
        self.persist_budget = None        # entries a durable queue's trim may take per step

    def _new_step(self):
        self.cur = defaultdict(bytes)
        self.ops, self.pubs, self.settles, self.gets = [], [], [], []

    # ---- topology
    def queue(self, name, L=None, mode=None, ttl=0, durable=False, **kw):
        lim = {}
        if L is not None and hasattr(self.dp, "queue_limits"):   # (the keywords exist with the feature)
            lim = dict(max_length=L, **({"overflow": mode} if mode else {}))
        slot = self.dp.declare_queue(VH, name, ttl_ms=ttl, durable=durable, **lim, **kw)
        self.q[name] = dict(slot=slot, L=L if self.on else None, mode=mode or "drop-head", ttl=ttl, durable=durable,
                            items=[], cons=None, serial=0)

    def open(self, conn, ch=1, confirm=False):
        if not any(c == conn for c, _ in self.chan):
            self.dp.open_connection(conn, VH)
        self.dp.open_channel(conn, ch)
        if confirm:
            self.dp.confirm_select(conn, ch)
        self.chan[(conn, ch)] = dict(confirm=confirm, pubs=0, tag=0, unacked=[], flow=True, win=[])

    def bind_fanout(self, q, exchange="amq.fanout"):
        self.dp.bind(VH, q, exchange, "")
        self.fan[exchange].append(q)

    def _consume(self, conn, ch, q, tag, no_ack, prefetch):
        self.q[q]["cons"] = dict(conn=conn, ch=ch, tag=tag, no_ack=no_ack, prefetch=prefetch)

    def consume(self, conn, ch, q, no_ack=True, prefetch=0, later=False):
        """``later``: attached by the control ops of the current step (before it runs)."""
        tag = "c-" + q
        calls = []
        if (conn, ch) not in self.chan:
            if not any(c == conn for c, _ in self.chan):
                calls.append(("open_connection", (conn, VH)))
            calls.append(("open_channel", (conn, ch)))
            self.chan[(conn, ch)] = dict(confirm=False, pubs=0, tag=0, unacked=[], flow=True, win=[])
        if prefetch:
            calls.append(("qos", (conn, ch), dict(prefetch_count=prefetch)))
        calls.append(("consume", (conn, ch, VH, q, tag), dict(no_ack=no_ack)))
        if later:
            self.ops += calls
        else:
            for c in calls:
                getattr(self.dp, c[0])(*c[1], **(c[2] if len(c) > 2 else {}))
        self._consume(conn, ch, q, tag, no_ack, prefetch)

    # ---- the current step
    def pub(self, conn, ch, n, q=None, exchange="", props=None, expire_ms=0):
        """n publishes to queue ``q`` through the default exchange, or to a fanout exchange."""
        name = q if q is not None else exchange
        src = self.q[q] if q is not None else self.fan
        for _ in range(n):
            if q is not None:
                i, src["serial"] = src["serial"], src["serial"] + 1
            else:
                i = self.seq
            body = body_of(name, i)
            p = dict(props or {})
            if expire_ms:
                p["expiration"] = str(expire_ms)
            self.cur[conn] += publish_command(ch, exchange, q or "", body, p or None)
            self.pubs.append((conn, len(self.pubs), ch, [q] if q is not None else sorted(self.fan[exchange]), body, expire_ms))
            self.seq += 1

    def ack_all(self, conn, ch):
        self.cur[conn] += ack_frame(ch, 0, multiple=True)
        self.settles.append((conn, ch, False))

    def nack_all(self, conn, ch):
        self.cur[conn] += nack(ch, 0)
        self.settles.append((conn, ch, True))

    def get(self, conn, ch, q, n=1):
        self.cur[conn] += get_cmd(ch, q, True) * n
        self.gets += [(conn, ch, q)] * n

    def flow(self, conn, ch, active):
        self.ops.append(("flow", (conn, ch, active)))
        self.chan[(conn, ch)]["flow"] = active

    # ---- the rules
    def end(self, n=1):
        for _ in range(n):
            self._end()

    def _end(self):
        k = len(self.steps)
        now = NOW + self.now_step_ms * k
        cnt = dict.fromkeys(COUNTERS, 0)
        ev = defaultdict(list)          # (conn, ch) -> [(kind, body, redelivered, tag)]
        empty = defaultdict(int)        # (conn, ch) -> Basic.GetEmpty frames
        # the window advance of the step: settled slots leave the channel's window (a no-ack
        # delivery is settled when it is made, and leaves with the next step)
        for c in self.chan.values():
            c["win"] = [s for s in c["win"] if s in [id(u[1]) for u in c["unacked"]]]
        # (1) enqueue, in publish order (connection, then wire order)
        failed = set()
        for conn, _, ch, qs, body, exp_ms in sorted(self.pubs, key=lambda p: p[:2]):
            self.chan[(conn, ch)]["pubs"] += 1
            for qn in qs:
                q = self.q[qn]
                if q["L"] is not None and q["mode"] == "reject-publish" and len(q["items"]) >= q["L"]:
                    cnt["n_maxlen_rejected"] += 1
                    failed.add((conn, ch))
                    continue
                exp = [e for e in (now + exp_ms if exp_ms else 0, now + q["ttl"] if q["ttl"] else 0) if e]
                q["items"].append(Entry(body, min(exp) if exp else 0, self.seq))
                self.seq += 1
        # (2) settles, then requeues: back in front of the heads, in their first order
        back = defaultdict(list)
        for conn, ch, requeue in self.settles:
            c = self.chan[(conn, ch)]
            for qn, e in c["unacked"]:
                if requeue:
                    back[qn].append(e)
                    cnt["n_requeue"] += 1
            c["unacked"] = []
            c["win"] = []
        for qn, es in back.items():
            for e in es:
                e.red = True
            self.q[qn]["items"][:0] = sorted(es, key=lambda e: e.seq)
        # (3) per queue, in slot order: TTL walk, Basic.Gets, dispatch, trim
        for qn, q in sorted(self.q.items(), key=lambda kv: kv[1]["slot"]):
            items = q["items"]
            while items and items[0].expire and items[0].expire <= now:
                items.pop(0)
                cnt["n_expired"] += 1
            for conn, ch, gq in self.gets:
                if gq != qn:
                    continue
                if not items:
                    empty[(conn, ch)] += 1
                    continue
                self._deliver(ev, cnt, conn, ch, "get_ok", None, qn, items.pop(0), True)
            c = q["cons"]
            if c is not None and items and self.chan[(c["conn"], c["ch"])]["flow"]:
                chan = self.chan[(c["conn"], c["ch"])]
                g = min(len(items), DELIVER_CAP)
                if not c["no_ack"] and c["prefetch"]:
                    g = min(g, max(c["prefetch"] - sum(1 for u in chan["unacked"] if u[0] == qn), 0))
                for e in items[:g]:
                    self._deliver(ev, cnt, c["conn"], c["ch"], "deliver", c["tag"], qn, e, c["no_ack"])
                del items[:g]
            if q["L"] is not None and q["mode"] == "drop-head" and len(items) > q["L"]:
                over = len(items) - q["L"]
                if q["durable"] and self.persist_budget is not None:
                    over = min(over, self.persist_budget)
                del items[:over]
                cnt["n_maxlen_dropped"] += over
        # (4) one confirm per confirm channel with publishes: Nack if one of them was refused
        conf = {}
        for key in sorted({(p[0], p[2]) for p in self.pubs}):
            c = self.chan[key]
            if c["confirm"]:
                n = sum(1 for p in self.pubs if (p[0], p[2]) == key)
                conf[key] = ("nack" if key in failed else "ack", c["pubs"], n > 1)
        inp = {c: b for c, b in self.cur.items()}
        if self.ops:
            inp["__ops__"] = self.ops
        self.steps.append(inp)
        self.want.append(dict(events=dict(ev), empty=dict(empty), confirms=conf, counters=cnt,
                              depth={q["slot"]: len(q["items"]) for q in self.q.values()}))
        self._new_step()

    def _deliver(self, ev, cnt, conn, ch, kind, ctag, qn, e, no_ack):
        chan = self.chan[(conn, ch)]
        chan["tag"] += 1
        chan["win"].append(id(e))
        assert len(chan["win"]) <= self.ucap, "scenario: the delivery window must not bind"
        if not no_ack:
            chan["unacked"].append((qn, e))
        ev[(conn, ch)].append((kind, ctag, e.body, e.red, chan["tag"]))
        cnt["n_deliv"] += 1


# ---------------------------------------------------------------- planes and runner
def cfg_of(sc, base):
    return dict(base, **sc.cfg)


def golden_plane(cfg, on=True):
    from chanamq_amd.engine.golden import GoldenDataPlane
    kw = {k: cfg[k] for k in GOLDEN_KEYS + ("ring_pool", "deliv_max", "egress_cap", "persist_max") if k in cfg}
    if cfg.get("persist"):
        kw["persist"] = True
    if on:
        kw["queue_limits"] = True
    return GoldenDataPlane(**kw)


def gpu_plane(cfg, graph, on=True):
    from chanamq_amd.engine.dataplane import GpuDataPlane
    return GpuDataPlane(graph=graph, **(dict(cfg, queue_limits=True) if on else cfg))


def persists(dp):
    return bool(dp.info.get("persist")) if hasattr(dp, "eng") else bool(dp.persist)


def persist_max(dp):
    return dp.info["persist_max"] if hasattr(dp, "eng") else dp.persist_max


def run_limits(dp, rec):
    """Drive dp through the record's steps (control ops first, the clock advanced per step)."""
    outs = []
    for k, inp in enumerate(rec.steps):
        inp = dict(inp)
        for op in inp.pop("__ops__", []):
            getattr(dp, op[0])(*op[1], **(op[2] if len(op) > 2 else {}))
        r = dp.step(inp, now_ms=NOW + rec.now_step_ms * k)
        if isinstance(r, dict):
            eg, ctrl, ev, segs, tx, cnt = r["egress"], r["ctrl"], r["events"], r["segs"], r.get("txbuf", []), r["counters"]
        else:
            eg, ctrl, ev, segs, tx, cnt = r.egress, r.ctrl, r.events, [s[:4] for s in r.segs], r.txbuf, r.counters
        o = dict(egress=eg, ctrl=sorted(ctrl), events=sorted(ev), gets=[], txbuf=sorted(tx),
                 segs=sorted((s[0], s[1], s[2], s[3]) for s in segs),
                 counters={c: int(cnt.get(c, 0)) for c in COUNTERS},
                 depth={q.slot: dp.message_count(q.slot) for q in dp.queues.values()})
        if persists(dp):   # store records: message ids differ between planes, the rest must not
            dp.take_persist()
            o["consumed"] = sorted((int(q), int(qpos), int(kind)) for _, q, qpos, kind in dp.take_consumed())
        outs.append(o)
    return outs


def observe(out, k):
    """One step's egress as the record states it: ({(conn, ch): [(kind, consumer tag, body,
    redelivered, delivery tag)]}, {(conn, ch): GetEmpty frames}, {(conn, ch): (ack | nack, tag,
    multiple)}).  Frames are parsed one by one; anything else on the wire fails here."""
    ev, empty, conf = defaultdict(list), defaultdict(int), {}
    for conn in sorted(out["egress"]):
        fp, cur = FrameParser(), None
        for fr in fp.feed(out["egress"][conn]):
            if fr.type == 1:
                assert cur is None, f"step {k} conn {conn}: method frame inside content"
                m = decode_method(fr.payload)
                if m.name == "basic.get_empty":
                    empty[(conn, fr.channel)] += 1
                elif m.name in ("basic.ack", "basic.nack"):
                    assert (conn, fr.channel) not in conf, f"step {k} conn {conn}: two confirms on one channel"
                    conf[(conn, fr.channel)] = (m.name[6:], m.delivery_tag, bool(m.multiple))
                else:
                    assert m.name in ("basic.deliver", "basic.get_ok"), f"step {k} conn {conn}: unexpected {m.name}"
                    cur = [fr.channel, m, None, []]
                continue
            assert cur is not None and fr.channel == cur[0], f"step {k} conn {conn}: stray content frame"
            if fr.type == 2:
                cur[2] = decode_content_header(fr.payload)[1]
            else:
                cur[3].append(fr.payload)
            if cur[2] is not None and sum(map(len, cur[3])) >= cur[2]:
                m, get = cur[1], cur[1].name == "basic.get_ok"
                ev[(conn, cur[0])].append(("get_ok" if get else "deliver", None if get else m.consumer_tag, b"".join(cur[3]),
                                           bool(m.redelivered), m.delivery_tag))
                cur = None
        assert cur is None and not fp.buf, f"step {k} conn {conn}: egress ends inside a command"
    return dict(ev), dict(empty), conf


def check(rec, outs):
    """The run against the record, step by step."""
    assert len(outs) == len(rec.want)
    for k, (o, w) in enumerate(zip(outs, rec.want)):
        ev, empty, conf = observe(o, k)
        assert conf == w["confirms"], f"step {k}: confirms {conf}, expected {w['confirms']}"
        assert ev == w["events"], f"step {k}: deliveries differ: got " \
            f"{ {c: [(e[0], e[2], e[3]) for e in v] for c, v in ev.items()} }, expected " \
            f"{ {c: [(e[0], e[2], e[3]) for e in v] for c, v in w['events'].items()} }"
        assert empty == w["empty"], f"step {k}: GetEmpty {empty}, expected {w['empty']}"
        assert o["counters"] == w["counters"], f"step {k}: counters {o['counters']}, expected {w['counters']}"
        assert o["depth"] == w["depth"], f"step {k}: depths {o['depth']}, expected {w['depth']}"
        if "consumed" in o:   # a trimmed persistent entry of a durable queue: one record, kind 1 (like an expired one)
            assert sum(1 for r in o["consumed"] if r[2] == 1) == w["counters"]["n_maxlen_dropped"] + w["counters"]["n_expired"]


# ---------------------------------------------------------------- scenarios
def sc_trim_waves(dp, on=True):
    """No consumer, L = 4.  Steps bring excesses of 1, 63, 64, 65 and 129 (one entry, a wave less
    one, a wave, a wave and one, two waves and one of the 64-entry walk); then a consumer drains:
    exactly the newest 4 of each step's state survive, in order."""
    r = Rec(dp, on)
    r.queue("tw", L=4)
    r.open(1)
    r.pub(1, 1, 5, "tw")
    r.end()
    for excess in (63, 64, 65, 129):
        r.pub(1, 1, excess, "tw")
        r.end()
    r.consume(2, 1, "tw", later=True)
    r.end(2)
    assert sum(w["counters"]["n_maxlen_dropped"] for w in r.want) == 1 + 63 + 64 + 65 + 129
    assert [e[2] for e in r.want[5]["events"][(2, 1)]] == [body_of("tw", i) for i in range(322, 326)]
    return r


def sc_trim_wrap(dp, on=True):
    """A 16-slot ring that cannot grow, L = 10, 6 arrivals a step (the ring holds L plus a step's
    arrivals exactly): head and tail wrap the ring several times, and the trim of the fifth
    step takes positions 14 .. 19, across the wrap."""
    r = Rec(dp, on)
    r.queue("wr", L=10, capacity=16, max_capacity=16)
    r.open(1, confirm=True)
    for _ in range(20):
        r.pub(1, 1, 6, "wr")
        r.end()
    r.consume(2, 1, "wr", later=True)
    r.end(2)
    assert all(w["confirms"][(1, 1)][0] == "ack" for w in r.want[:20])
    assert [e[2] for e in r.want[20]["events"][(2, 1)]] == [body_of("wr", i) for i in range(110, 120)]
    return r


def sc_trim_zero(dp, on=True):
    """L = 0: nothing stays queued, and consumers and Gets still take what the step brought.  A
    prefetch-3 consumer gets 3 of 5 and the other 2 go; without a consumer all 5 go, a Get in
    the same step takes the oldest first, and a later Get finds the queue empty."""
    r = Rec(dp, on)
    r.queue("z3", L=0)
    r.queue("z0", L=0)
    r.open(1)
    r.open(3)
    r.consume(2, 1, "z3", no_ack=False, prefetch=3)
    r.pub(1, 1, 5, "z3")
    r.pub(1, 1, 5, "z0")
    r.end()
    r.ack_all(2, 1)
    r.pub(1, 1, 2, "z3")
    r.pub(1, 1, 3, "z0")
    r.get(3, 1, "z0")
    r.end()
    r.get(3, 1, "z0")
    r.ack_all(2, 1)
    r.end(2)
    assert [w["counters"]["n_maxlen_dropped"] for w in r.want] == [7, 2, 0, 0]
    assert r.want[1]["events"][(3, 1)][0][2] == body_of("z0", 5) and r.want[2]["empty"] == {(3, 1): 1}
    return r


def sc_after_dispatch(dp, on=True):
    """L = 2, a manual-ack consumer with prefetch 3, 10 arrive: positions 0-2 are delivered, 3-7
    trimmed, 8-9 kept, and after the acks the next step delivers 8 and 9.  In the same step a
    Basic.Get on a second limited queue is served (the oldest entry) before that queue's trim."""
    r = Rec(dp, on)
    r.queue("ad", L=2)
    r.queue("ag", L=2)
    r.open(1)
    r.open(3)
    r.consume(2, 1, "ad", no_ack=False, prefetch=3)
    r.pub(1, 1, 2, "ag")
    r.end()
    r.pub(1, 1, 10, "ad")
    r.pub(1, 1, 3, "ag")
    r.get(3, 1, "ag")
    r.end()
    r.ack_all(2, 1)
    r.end()
    r.get(3, 1, "ag", 2)
    r.ack_all(2, 1)
    r.end(2)
    w = r.want
    assert [e[2] for e in w[1]["events"][(2, 1)]] == [body_of("ad", i) for i in (0, 1, 2)]
    assert w[1]["events"][(3, 1)][0][2] == body_of("ag", 0) and w[1]["counters"]["n_maxlen_dropped"] == 5 + 2
    assert [e[2] for e in w[2]["events"][(2, 1)]] == [body_of("ad", i) for i in (8, 9)]
    assert [e[2] for e in w[3]["events"][(3, 1)]] == [body_of("ag", i) for i in (3, 4)]
    return r


TTL_STEP_MS = 600


def sc_ttl_then_trim(dp, on=True):
    """Queue ttl 1000 ms, 600 ms a step, L = 3.  Three entries expire at the head in the step
    that brings 6 more: the TTL walk takes the 3, the trim 3 of the 6; each counter is exact."""
    r = Rec(dp, on, TTL_STEP_MS)
    r.queue("tt", L=3, ttl=1000)
    r.open(1)
    r.pub(1, 1, 5, "tt")
    r.end(2)
    r.pub(1, 1, 6, "tt")
    r.end()
    r.consume(2, 1, "tt", later=True)
    r.end(2)
    assert [(w["counters"]["n_expired"], w["counters"]["n_maxlen_dropped"]) for w in r.want[:3]] == [(0, 2), (0, 0), (3, 3)]
    assert [e[2] for e in r.want[3]["events"][(2, 1)]] == [body_of("tt", i) for i in (8, 9, 10)]
    return r


def sc_requeue_over(dp, on=True):
    """Nack-requeue of 3 into a drop-head queue at L = 4.  The requeued 3 are the oldest: where
    the requeuing consumer has credit (queue ra) it gets them again, flagged; where it has none
    (queue rb: its channel's flow is off) they are trimmed first and the 4 newer ones stay."""
    r = Rec(dp, on)
    r.open(1)
    for q, conn in (("ra", 2), ("rb", 3)):
        r.queue(q, L=4)
        r.consume(conn, 1, q, no_ack=False, prefetch=3)
        r.pub(1, 1, 3, q)
    r.end()
    r.pub(1, 1, 4, "ra")
    r.pub(1, 1, 4, "rb")
    r.end()
    r.nack_all(2, 1)
    r.nack_all(3, 1)
    r.flow(3, 1, False)
    r.end()
    r.flow(3, 1, True)
    r.ack_all(2, 1)
    r.end()
    for _ in range(3):
        r.ack_all(2, 1)
        r.ack_all(3, 1)
        r.end()
    w = r.want
    assert [(e[2], e[3]) for e in w[2]["events"][(2, 1)]] == [(body_of("ra", i), True) for i in range(3)]
    assert (3, 1) not in w[2]["events"] and w[2]["counters"]["n_maxlen_dropped"] == 3
    assert [(e[2], e[3]) for e in w[3]["events"][(3, 1)]] == [(body_of("rb", i), False) for i in (3, 4, 5)]
    return r


def sc_grow_to_limit(dp, on=True):
    """Capacity 16, L = 100, 300 in one step: the ring grows to hold L plus the step's arrivals,
    100 are left and nothing is nacked."""
    r = Rec(dp, on)
    r.queue("gl", L=100, capacity=16)
    r.open(1, confirm=True)
    r.pub(1, 1, 300, "gl")
    r.end()
    r.consume(2, 1, "gl", later=True)
    r.end(2)
    assert r.want[0]["confirms"] == {(1, 1): ("ack", 300, True)} and r.want[0]["counters"]["n_maxlen_dropped"] == 200
    assert [e[2] for e in r.want[1]["events"][(2, 1)]] == [body_of("gl", i) for i in range(200, 300)]
    return r


def sc_reject_basic(dp, on=True):
    """L = 4, reject-publish, a confirm channel: 2 fit (Ack), of 10 in one step 2 are stored and 8
    refused (Nack), one more is refused alone; after a drain the queue takes publishes again."""
    r = Rec(dp, on)
    r.queue("rj", L=4, mode="reject-publish")
    r.open(1, confirm=True)
    r.pub(1, 1, 2, "rj")
    r.end()
    r.pub(1, 1, 10, "rj")
    r.end()
    r.pub(1, 1, 1, "rj")
    r.end()
    r.consume(2, 1, "rj", later=True)
    r.end()
    r.pub(1, 1, 3, "rj")
    r.end(2)
    w = r.want
    assert [x["confirms"].get((1, 1)) for x in w[:5]] == [("ack", 2, True), ("nack", 12, True), ("nack", 13, False), None,
                                                         ("ack", 16, True)]
    assert [x["counters"]["n_maxlen_rejected"] for x in w[:3]] == [0, 8, 1]
    assert [e[2] for e in w[3]["events"][(2, 1)]] == [body_of("rj", i) for i in (0, 1, 2, 3)]
    return r


def sc_reject_fanout(dp, on=True):
    """A fanout to a full limited queue and an unlimited one: the unlimited queue gets every
    message, the refusals release their references (nothing leaks, nothing is freed twice)."""
    r = Rec(dp, on)
    r.queue("ff", L=2, mode="reject-publish")
    r.queue("fu")
    r.bind_fanout("ff")
    r.bind_fanout("fu")
    r.open(1, confirm=True)
    r.pub(1, 1, 6, exchange="amq.fanout")
    r.end()
    r.pub(1, 1, 3, exchange="amq.fanout")
    r.consume(2, 1, "ff", later=True)
    r.consume(2, 2, "fu", later=True)
    r.end(3)
    w = r.want
    assert [x["counters"]["n_maxlen_rejected"] for x in w[:2]] == [4, 3] and w[1]["confirms"] == {(1, 1): ("nack", 9, True)}
    assert len(w[1]["events"][(2, 1)]) == 2 and len(w[1]["events"][(2, 2)]) == 9
    return r


def sc_reject_requeue_over(dp, on=True):
    """3 requeues into a full reject-publish queue (L = 3) whose consumer's flow is off: they are
    accepted and the depth is 6.  The 2 publishes of the same step are refused (the queue was
    full before the requeue), and so are the 2 of the next step: the room is zero, not 2^64 - 3."""
    r = Rec(dp, on)
    r.queue("rr", L=3, mode="reject-publish")
    r.open(1, confirm=True)
    r.consume(2, 1, "rr", no_ack=False, prefetch=3)
    r.pub(1, 1, 3, "rr")
    r.end()
    r.pub(1, 1, 3, "rr")
    r.end()
    r.nack_all(2, 1)
    r.flow(2, 1, False)
    r.pub(1, 1, 2, "rr")
    r.end()
    r.pub(1, 1, 2, "rr")
    r.end()
    r.flow(2, 1, True)
    r.end()
    for _ in range(3):
        r.ack_all(2, 1)
        r.end()
    w = r.want
    assert [x["counters"]["n_maxlen_rejected"] for x in w[:4]] == [0, 0, 2, 2] and w[3]["depth"] == {0: 6}
    assert [(e[2], e[3]) for e in w[4]["events"][(2, 1)]] == [(body_of("rr", i), True) for i in range(3)]
    return r


def sc_reject_at_capacity(dp, on=True):
    """Reject-publish where the ring has exactly as much room as the limit, so that ring and limit
    end at the same pair: the refusal is the limit's (`n_maxlen_rejected`, never `n_ring_full`).
    Queue rc starts there (a 16-slot ring that cannot grow, L = 16).  Queue rg grows to it: 17
    arrivals move its 16-slot ring to 64 = L, 60 more fill it (47 stored, 13 refused).  Queue rq is
    filled by a requeue: L = 8 in a 16-slot ring that cannot grow, 8 ready and 8 requeued (the
    consumer's flow off) make its depth the capacity, and the room and the ring's are both zero."""
    r = Rec(dp, on)
    r.queue("rc", L=16, mode="reject-publish", capacity=16, max_capacity=16)
    r.queue("rg", L=64, mode="reject-publish", capacity=16)
    r.queue("rq", L=8, mode="reject-publish", capacity=16, max_capacity=16)
    r.open(1, confirm=True)
    r.consume(3, 1, "rq", no_ack=False, prefetch=8)
    r.pub(1, 1, 10, "rc")
    r.pub(1, 1, 17, "rg")
    r.pub(1, 1, 8, "rq")
    r.end()
    r.pub(1, 1, 10, "rc")
    r.pub(1, 1, 60, "rg")
    r.pub(1, 1, 8, "rq")
    r.end()
    r.nack_all(3, 1)
    r.flow(3, 1, False)
    r.pub(1, 1, 3, "rc")
    r.pub(1, 1, 5, "rg")
    r.end()
    r.pub(1, 1, 2, "rq")
    r.end()
    r.flow(3, 1, True)
    r.consume(2, 1, "rc", later=True)
    r.consume(2, 2, "rg", later=True)
    r.end()
    for _ in range(3):
        r.ack_all(3, 1)
        r.end()
    w = r.want
    assert [x["counters"]["n_maxlen_rejected"] for x in w[:4]] == [0, 4 + 13, 3 + 5, 2]
    assert all(x["counters"]["n_ring_full"] == 0 for x in w)
    assert w[3]["depth"] == {0: 16, 1: 64, 2: 16} and w[3]["confirms"] == {(1, 1): ("nack", 123, True)}
    assert len(w[4]["events"][(2, 1)]) == 16 and len(w[4]["events"][(2, 2)]) == 64
    return r


DURABLE_L = 50
# the engine never runs with persist_max below 2 * deliv_max + 4096 (a step's records always fit),
# so a quarter of it -- the budget the TTL walk and the trim share -- is 1280 here, the smallest
# this configuration allows: 20 reservations of 64, of which the TTL walk of a queue that is not
# empty takes one.  An excess of 150 is trimmed in one step; 2600 take three
DURABLE_CFG = dict(persist=1, persist_max=4096, persist_bytes=8 << 20, deliv_max=512, pair_max=4096)
DURABLE_EXCESS = (150, 2600)


def sc_durable_budget(dp, on=True):
    """A persisting plane, one durable queue, persistent publishes.  The trim draws on the TTL
    walk's record budget, so the large excess goes over three steps (1216, 1216, 168); then the
    depth is L and stays."""
    r = Rec(dp, on)
    assert persists(dp) and (persist_max(dp) >> 2) == 1280
    r.persist_budget = ((persist_max(dp) >> 2) // 64 - 1) * 64
    r.queue("du", L=DURABLE_L, durable=True)
    r.open(1)
    r.pub(1, 1, DURABLE_L + DURABLE_EXCESS[0], "du", props=PERSISTENT)
    r.end()
    r.pub(1, 1, DURABLE_EXCESS[1], "du", props=PERSISTENT)
    r.end(5)
    r.consume(2, 1, "du", later=True)
    r.end(2)
    assert [w["counters"]["n_maxlen_dropped"] for w in r.want[:6]] == [150, 1216, 1216, 168, 0, 0]
    assert [w["depth"][0] for w in r.want[3:6]] == [DURABLE_L] * 3
    return r


def sc_off(dp, on=False):
    """The same declares with the option off: 10 stay in an x-max-length = 2 queue, a
    reject-publish queue takes 10 and confirms with Ack, neither counter moves."""
    r = Rec(dp, False)
    r.queue("od", L=2)
    r.queue("oj", L=2, mode="reject-publish")
    r.open(1, confirm=True)
    r.pub(1, 1, 10, "od")
    r.pub(1, 1, 10, "oj")
    r.end()
    r.consume(2, 1, "od", later=True)
    r.consume(2, 2, "oj", later=True)
    r.end(2)
    assert r.want[0]["confirms"] == {(1, 1): ("ack", 20, True)} and r.want[0]["depth"] == {0: 10, 1: 10}
    assert all(not w["counters"]["n_maxlen_dropped"] and not w["counters"]["n_maxlen_rejected"] for w in r.want)
    return r


TWO_PASS = dict(q_max=4096)    # a pair key above SORT_ONEPASS_BITS: k_ring_plan + k_enqueue instead of the fused sort
SCENARIOS = {
    "trim_waves": Scenario(sc_trim_waves, {}, 0, True),
    "trim_wrap": Scenario(sc_trim_wrap, {}, 0, True),
    "trim_zero": Scenario(sc_trim_zero, {}, 0, True),
    "after_dispatch": Scenario(sc_after_dispatch, {}, 0, True),
    "ttl_then_trim": Scenario(sc_ttl_then_trim, {}, TTL_STEP_MS, True),
    "requeue_over": Scenario(sc_requeue_over, {}, 0, True),
    "grow_to_limit": Scenario(sc_grow_to_limit, {}, 0, True),
    "reject_basic": Scenario(sc_reject_basic, {}, 0, True),
    "reject_fanout": Scenario(sc_reject_fanout, {}, 0, True),
    "reject_requeue_over": Scenario(sc_reject_requeue_over, {}, 0, True),
    # both_paths: the reject and grow scenarios again at the two-pass key width
    "both_paths_reject_basic": Scenario(sc_reject_basic, TWO_PASS, 0, True),
    "both_paths_reject_requeue_over": Scenario(sc_reject_requeue_over, TWO_PASS, 0, True),
    "both_paths_grow_to_limit": Scenario(sc_grow_to_limit, TWO_PASS, 0, True),
    "reject_at_capacity": Scenario(sc_reject_at_capacity, {}, 0, True),
    "both_paths_reject_at_capacity": Scenario(sc_reject_at_capacity, TWO_PASS, 0, True),
    "durable_budget": Scenario(sc_durable_budget, DURABLE_CFG, 0, True),
}
OFF = Scenario(sc_off, {}, 0, True)


# ================================================================ sharded
# a drop-head and a reject-publish queue owned by rank 1, published from rank 0 on a confirm
# channel: the owner trims / refuses, the publisher gets Basic.Ack (as for a remote full ring)
SHARD_STEPS, SHARD_N = 6, 8
SHARD_QUEUES = (("sd", 3, "drop-head"), ("sj", 2, "reject-publish"))
PUB_CONN, CONS_CONN = 1, 10


def sharded_cluster(cfg, lag=0, gpu=False, graph=True):
    from chanamq_amd.parallel.cluster import LocalCluster
    from xchg_scenarios import golden_kw
    if gpu:
        import torch

        from chanamq_amd.engine.dataplane import GpuDataPlane
        torch.cuda.set_device(0)
        return LocalCluster(lambda **k: GpuDataPlane(graph=graph, exchange_lag=lag, queue_limits=True, **cfg, **k), 2)
    from chanamq_amd.engine.golden import GoldenDataPlane
    return LocalCluster(lambda **k: GoldenDataPlane(exchange_lag=lag, queue_limits=True, **golden_kw(cfg), **k), 2)


def sharded_run(cl, now=NOW):
    """-> per rank and step (egress by connection, the two counters)."""
    for q, _, _ in SHARD_QUEUES:
        cl.shard_map.place(VH, q, 1)
    for p in cl.planes:
        for q, L, mode in SHARD_QUEUES:
            p.declare_queue(VH, q, capacity=64, max_length=L, overflow=mode)
    cl[0].open_connection(PUB_CONN, VH)
    cl[0].open_channel(PUB_CONN, 1)
    cl[0].confirm_select(PUB_CONN, 1)
    data = b"".join(publish_command(1, "", q, body_of(q, i)) for q, _, _ in SHARD_QUEUES for i in range(SHARD_N))
    outs = [[] for _ in range(2)]
    for k in range(SHARD_STEPS):
        if k == 3:   # once the owner has imported, trimmed and refused: its consumers attach
            cl[1].open_connection(CONS_CONN, VH)
            cl[1].open_channel(CONS_CONN, 1)
            for q, _, _ in SHARD_QUEUES:
                cl[1].consume(CONS_CONN, 1, VH, q, "c-" + q, no_ack=True)
        res = cl.step([{PUB_CONN: data} if k == 0 else {}, {}], now_ms=now + k)
        for r, o in enumerate(res):
            eg, cnt = (o["egress"], o["counters"]) if isinstance(o, dict) else (o.egress, o.counters)
            outs[r].append((dict(eg), int(cnt.get("n_maxlen_dropped", 0)), int(cnt.get("n_maxlen_rejected", 0))))
    return outs


def sharded_check(outs):
    """What the rules say, from the wire: Acks only on the publisher's rank, the newest 3 of the
    drop-head queue and the first 2 of the reject-publish queue on the owner's."""
    conf, got = [], defaultdict(list)
    for r in range(2):
        for k, (eg, _, _) in enumerate(outs[r]):
            ev, empty, c = observe(dict(egress=eg), k)
            conf += [(r, key, v) for key, v in c.items()]
            for key, es in ev.items():
                assert r == 1 and key == (CONS_CONN, 1)
                for e in es:
                    got[e[1]].append(e[2])
    assert conf == [(0, (PUB_CONN, 1), ("ack", 2 * SHARD_N, True))]
    assert dict(got) == {"c-sd": [body_of("sd", i) for i in range(SHARD_N - 3, SHARD_N)],
                         "c-sj": [body_of("sj", i) for i in range(2)]}
    assert [sum(o[1] for o in outs[r]) for r in (0, 1)] == [0, SHARD_N - 3]
    assert [sum(o[2] for o in outs[r]) for r in (0, 1)] == [0, SHARD_N - 2]
