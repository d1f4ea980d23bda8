"""Queue byte limits (x-max-length-bytes, ``queue_limit_bytes=True`` on top of
``queue_limits=True``) in the ``limit_scenarios`` style: each scenario is ``(dp, on) -> BRec`` with
its own engine overrides on top of ``gpu_cfg.CFG``.

``BRec`` is the scenarios' own record: a plain Python list per queue, to which it applies the rule
as CHANGES.md "Queue byte limits on the GPU path" states it.

* Ready bytes are the body bytes of a queue's list.
* reject-publish: with the queue's pairs of the step in publish order, Y the ready bytes before
  the step's enqueue and E_r the body sizes of the pairs before pair r, pair r passes iff
  Y + E_r < B; K is the number that pass; a pair is stored iff its rank is below
  min(ring room, count room, K); a refusal is the limit's when min(count room, K) <= ring room,
  else the ring's.  Requeues are never refused.
* drop-head: at the end of the queue's step, entries leave the head while depth > L or ready
  bytes > B, 64 an iteration, a durable queue on a persisting plane paying one reservation of
  the TTL walk's budget per iteration.

While a scenario is written, the record builds the wire input of every step and predicts what the
step must put on the wire, the depths and ready bytes it leaves and the step's counters.  It never
looks at the golden model: ``check`` judges the golden model's run and the HIP data plane's alike.
"""

from collections import defaultdict

from chanamq_amd.engine.traffic import publish_command
from consumer_scenarios import GOLDEN_KEYS, body_of
from dp_scenarios import NOW, VH
from limit_scenarios import (COUNTERS, DELIVER_CAP, DURABLE_CFG, PERSISTENT, TWO_PASS, Entry, Rec, Scenario, observe, persist_max,
                             persists)
from limit_scenarios import check as check_limits

INF = float("inf")
SORT_TILE = 1024   # dp_state.h: the radix sort's tile


def sized(name, i, size):
    """The i-th message of ``name`` with a body of exactly ``size`` bytes."""
    return body_of(name, i, size)[:size]


class BRec(Rec):
    """``Rec`` with body sizes, ring room, the byte rule and dead-lettering of what a trim takes.
    ``on``: the byte flag (the count limit is always on here)."""

    def __init__(self, dp, on=True, now_step_ms=0, ucap=256):
        super().__init__(dp, True, now_step_ms, ucap)
        self.bytes_on = on
        self.dead, self.died = [], []   # dead letters awaiting the next step's pass: (target queue, body)

    # ---- topology
    def queue(self, name, L=None, B=None, mode=None, ttl=0, durable=False, cap=None, keep=None, dlq=None, later=False,
              slot=None):
        """``cap``: a ring of exactly that many slots that cannot grow; ``keep``: a ring of that many
        slots that may grow and is expected not to; ``dlq``: the queue that the dead-letter
        exchange (amq.fanout) feeds; ``later``: declared by the control ops of the current step,
        into ``slot``."""
        kw = dict(ttl_ms=ttl, durable=durable)
        if L is not None:
            kw["max_length"] = L
        if B is not None:
            kw["max_length_bytes"] = B
        if mode:
            kw["overflow"] = mode
        if cap:
            kw.update(capacity=cap, max_capacity=cap)
        if keep:
            kw.update(capacity=keep)
        if dlq:
            kw["dead_letter_exchange"] = "amq.fanout"
        if later:
            self.ops.append(("declare_queue", (VH, name), kw))
        else:
            slot = self.dp.declare_queue(VH, name, **kw)
        self.q[name] = dict(slot=slot, L=L, B=B if self.bytes_on else None, mode=mode or "drop-head", ttl=ttl,
                            durable=durable, items=[], cons=None, serial=0, cap=cap, keep=keep, dlq=dlq)

    def delete(self, name):
        """Queue.Delete by the control ops of the current step; the entries go with the queue."""
        self.ops.append(("delete_queue", (VH, name)))
        return self.q.pop(name)["slot"]

    def purge(self, name):
        """Queue.Purge between steps: the entries are marked expired (expiry 1) and still count,
        in depth and bytes, until the next step's TTL walk."""
        self.ops.append(("purge", (self.q[name]["slot"],)))
        for e in self.q[name]["items"]:
            e.expire = 1

    def get_between(self, conn, ch, name):
        """Basic.Get (no-ack) between steps, on a channel that carries nothing else: expired
        entries at the head go first, then the head entry is handed out."""
        k = len(self.steps)
        now = NOW + self.now_step_ms * k
        self.ops.append(("basic_get", (conn, ch, self.q[name]["slot"], True, now)))
        items = self.q[name]["items"]
        while items and items[0].expire and items[0].expire <= now:
            items.pop(0)
        if items:
            items.pop(0)
            self.chan[(conn, ch)]["tag"] += 1

    # ---- the current step
    def pub(self, conn, ch, sizes, q=None, exchange="", props=None, expire_ms=0):
        """One publish per entry of ``sizes`` (body bytes) to queue ``q`` through the default
        exchange, or to a fanout exchange."""
        name = q if q is not None else exchange
        for size in sizes:
            if q is not None:
                i, self.q[q]["serial"] = self.q[q]["serial"], self.q[q]["serial"] + 1
            else:
                i = self.seq
            body = sized(name, i, size)
            p = dict(props or {})
            if expire_ms:
                p["expiration"] = str(expire_ms)
            self.cur[conn] += publish_command(ch, exchange, q or "", body, p or None)
            self.pubs.append((conn, len(self.pubs), ch, [q] if q is not None else sorted(self.fan[exchange]), body, expire_ms))
            self.seq += 1

    # ---- the rules
    @staticmethod
    def ready_bytes(q):
        return sum(len(e.body) for e in q["items"])

    def _end(self):
        k = len(self.steps)
        now = NOW + self.now_step_ms * k
        cnt = dict.fromkeys(COUNTERS, 0)
        ev = defaultdict(list)
        empty = defaultdict(int)
        for c in self.chan.values():
            c["win"] = [s for s in c["win"] if s in [id(u[1]) for u in c["unacked"]]]
        # (1) enqueue: the step's pairs per queue, in publish order (connection, then wire order),
        # the dead letters of the last step behind them
        pairs = defaultdict(list)
        for conn, _, ch, qs, body, exp_ms in sorted(self.pubs, key=lambda p: p[:2]):
            self.chan[(conn, ch)]["pubs"] += 1
            for qn in qs:
                pairs[qn].append(((conn, ch), body, exp_ms))
        for qn, body in self.dead:
            pairs[qn].append((None, body, 0))
        self.dead = []
        failed = set()
        for qn, ps in pairs.items():
            q = self.q[qn]
            depth, reject = len(q["items"]), q["mode"] == "reject-publish"
            ring_room = q["cap"] - depth if q["cap"] else INF
            count_room = max(q["L"] - depth, 0) if reject and q["L"] is not None else INF
            K = INF
            if reject and q["B"] is not None:
                y, K = self.ready_bytes(q), 0
                for _, body, _ in ps:
                    if not y < q["B"]:
                        break
                    K += 1
                    y += len(body)
            lim = min(count_room, K)
            for rank, (key, body, exp_ms) in enumerate(ps):
                if rank < min(ring_room, lim):
                    exp = [e for e in (now + exp_ms if exp_ms else 0, now + q["ttl"] if q["ttl"] else 0) if e]
                    q["items"].append(Entry(body, min(exp) if exp else 0, self.seq))
                    self.seq += 1
                    continue
                cnt["n_maxlen_rejected" if lim <= ring_room else "n_ring_full"] += 1
                if key is not None:
                    failed.add(key)
        # (2) settles, then requeues: back in front of the heads, in their first order (never refused)
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
        budget = self.persist_budget   # 64-entry reservations the step's durable walks share
        for qn, q in sorted(self.q.items(), key=lambda kv: kv[1]["slot"]):
            items = q["items"]
            paying = q["durable"] and budget is not None
            if paying and items:   # the TTL walk's look at a head that is not empty: one reservation
                budget -= 1
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
                g = min(len(items), DELIVER_CAP, self.ucap - len(chan["win"]))   # (one consumer a channel here)
                if not c["no_ack"] and c["prefetch"]:
                    g = min(g, max(c["prefetch"] - sum(1 for u in chan["unacked"] if u[0] == qn), 0))
                for e in items[:g]:
                    self._deliver(ev, cnt, c["conn"], c["ch"], "deliver", c["tag"], qn, e, c["no_ack"])
                del items[:g]
            if q["mode"] != "drop-head":
                continue

            def over():
                return (q["L"] is not None and len(items) > q["L"]) or (q["B"] is not None and self.ready_bytes(q) > q["B"])
            while over():
                if paying:
                    if budget <= 0:
                        break
                    budget -= 1
                for _ in range(64):
                    if not over():
                        break
                    e = items.pop(0)
                    cnt["n_maxlen_dropped"] += 1
                    if q["dlq"] and e.expire != 1:
                        self.dead.append((q["dlq"], e.body))
                        self.died.append(e.body)
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
                              depth={q["slot"]: len(q["items"]) for q in self.q.values()},
                              bytes={q["slot"]: self.ready_bytes(q) for q in self.q.values()},
                              cap={q["slot"]: q["cap"] or q["keep"] for q in self.q.values() if q["cap"] or q["keep"]}))
        self._new_step()


# ---------------------------------------------------------------- planes and runner
def cfg_of(sc, base):
    return dict(base, **sc.cfg)


DL_KEYS = ("dead_max", "dead_bytes", "restore_max")


def plane_kw(cfg, on):
    kw = dict(queue_limits=True)
    if on:
        kw["queue_limit_bytes"] = True
    for k in ("dead_letter", "x_death"):
        if cfg.get(k):
            kw[k] = True
    return kw


def golden_plane(cfg, on=True):
    from chanamq_amd.engine.golden import GoldenDataPlane
    kw = {k: cfg[k] for k in GOLDEN_KEYS + ("ring_pool", "deliv_max", "egress_cap", "persist_max") + DL_KEYS if k in cfg}
    if cfg.get("persist"):
        kw["persist"] = True
    return GoldenDataPlane(**kw, **plane_kw(cfg, on))


def gpu_plane(cfg, graph, on=True):
    from chanamq_amd.engine.dataplane import GpuDataPlane
    return GpuDataPlane(graph=graph, **dict(cfg, **plane_kw(cfg, on)))


def ring_capacity(dp, q):
    """The queue's ring capacity as the plane holds it now (a growth moves it)."""
    if hasattr(dp, "eng"):
        return dp._u64("q_ring_mask", q.slot) + 1
    return q.capacity


def run_bytes(dp, rec):
    """``limit_scenarios.run_limits`` with the ready bytes and the ring capacity of every queue
    after each step."""
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
                 depth={q.slot: dp.message_count(q.slot) for q in dp.queues.values()},
                 cap={q.slot: int(ring_capacity(dp, q)) for q in dp.queues.values()})
        if getattr(dp, "queue_limit_bytes", False):
            o["bytes"] = {q.slot: int(dp.queue_bytes(q.slot)) for q in dp.queues.values()}
        if persists(dp):   # store records: message ids differ between planes, the rest must not
            dp.take_persist()
            o["consumed"] = sorted((int(q), int(qpos), int(kind)) for _, q, qpos, kind in dp.take_consumed())
        outs.append(o)
    return outs


def check(rec, outs):
    """The run against the record, step by step: what ``limit_scenarios.check`` holds, then the
    ready bytes of every queue and the capacity of every ring that must not grow."""
    check_limits(rec, outs)
    for k, (o, w) in enumerate(zip(outs, rec.want)):
        if "bytes" in o:
            assert o["bytes"] == w["bytes"], f"step {k}: ready bytes {o['bytes']}, expected {w['bytes']}"
        for slot, cap in w["cap"].items():
            assert o["cap"][slot] == cap, f"step {k}: ring of slot {slot} holds {o['cap'][slot]}, expected {cap}"


# ---------------------------------------------------------------- scenarios
def sc_trim_wave_edges(dp, on=True):
    """A drop-head queue, B = 40 bytes, bodies of 10: four stay.  Steps bring byte excesses that
    trim 63, 64, 65 and 129 entries (a wave less one, a wave, a wave and one, two waves and one of
    the 64-entry walk); a consumer then drains the newest four."""
    r = BRec(dp, on)
    r.queue("we", B=40)
    r.open(1)
    r.pub(1, 1, [10] * 4, "we")
    r.end()
    for excess in (63, 64, 65, 129):
        r.pub(1, 1, [10] * excess, "we")
        r.end()
    r.consume(2, 1, "we", later=True)
    r.end(2)
    assert [w["counters"]["n_maxlen_dropped"] for w in r.want[:5]] == [0, 63, 64, 65, 129]
    assert all(w["bytes"] == {0: 40} for w in r.want[:5])
    assert [e[2] for e in r.want[5]["events"][(2, 1)]] == [sized("we", i, 10) for i in range(321, 325)]
    return r


def sc_trim_sizes(dp, on=True):
    """Bodies of 0 bytes at the head: they leave only while the bytes behind them are over (an
    empty body before a live excess goes, one at the head of a queue within B stays).  One body
    larger than B alone: the queue ends empty.  B = 0: only empty bodies stay."""
    r = BRec(dp, on)
    r.queue("ts", B=100)
    r.queue("tz", B=0)
    r.open(1)
    r.pub(1, 1, [0, 0, 60, 0, 50, 0, 30], "ts")   # 140: the two empties and the 60 go (80 left, a 0 at the head)
    r.pub(1, 1, [0, 5, 0], "tz")                  # 5 > 0: the empty and the 5 go, the last empty stays
    r.end()
    r.pub(1, 1, [101], "ts")                      # 181, then 131, 131, 101, 101: everything goes
    r.pub(1, 1, [0, 0], "tz")
    r.end()
    r.pub(1, 1, [100], "ts")                      # exactly B: stays
    r.end()
    r.consume(2, 1, "ts", later=True)
    r.consume(2, 2, "tz", later=True)
    r.end(2)
    w = r.want
    assert [x["counters"]["n_maxlen_dropped"] for x in w[:3]] == [3 + 2, 5, 0]
    assert [x["depth"] for x in w[:3]] == [{0: 4, 1: 1}, {0: 0, 1: 3}, {0: 1, 1: 3}]
    assert [x["bytes"] for x in w[:3]] == [{0: 80, 1: 0}, {0: 0, 1: 0}, {0: 100, 1: 0}]
    return r


def sc_both_limits(dp, on=True):
    """L = 50 and B = 1000 together.  Step 0: 80 bodies of 10 -- the count binds (30 go, 500
    bytes).  Step 1: 10 bodies of 100 -- the bytes bind (1500 -> 1000: 50 of the 10s go, the
    count is 10).  Step 2, both inside one 64-entry iteration: 45 bodies of 1 make 55 entries of
    1045 bytes; the first entry (100) satisfies the bytes, the count takes four more."""
    r = BRec(dp, on)
    r.queue("bl", L=50, B=1000)
    r.open(1)
    r.pub(1, 1, [10] * 80, "bl")
    r.end()
    r.pub(1, 1, [100] * 10, "bl")
    r.end()
    r.pub(1, 1, [1] * 45, "bl")
    r.end()
    r.consume(2, 1, "bl", later=True)
    r.end(2)
    w = r.want
    assert [x["counters"]["n_maxlen_dropped"] for x in w[:3]] == [30, 50, 5]
    assert [(x["depth"][0], x["bytes"][0]) for x in w[:3]] == [(50, 500), (10, 1000), (50, 545)]
    return r


OVERSIZE = 500


def sc_reject_prefix(dp, on=True):
    """reject-publish, B = 200, a confirm channel per case so that every Nack range is checked.
    rp0: full before the step (K = 0).  rp1: empty, an oversize body first -- accepted, the next
    pair refused (K = 1).  rpm: mixed sizes 0, 1, 100, 100 (reaching 201), then refused (K = 4 of
    7).  rpa: everything fits below B until the last pair (K = cnt)."""
    r = BRec(dp, on)
    for i, q in enumerate(("rp0", "rp1", "rpm", "rpa")):
        r.queue(q, B=200, mode="reject-publish")
        r.open(1 + i, confirm=True)
    r.pub(1, 1, [100, 100], "rp0")
    r.end()
    r.pub(1, 1, [0, 1, 100], "rp0")
    r.pub(2, 1, [OVERSIZE, 0, 1], "rp1")
    r.pub(3, 1, [0, 1, 100, 100, 0, 1, OVERSIZE], "rpm")
    r.pub(4, 1, [0, 1, 100, 98, OVERSIZE], "rpa")
    r.end()
    r.pub(4, 1, [0], "rpa")
    r.end()
    for i, q in enumerate(("rp0", "rp1", "rpm", "rpa")):
        r.consume(10, 1 + i, q, later=True)
    r.end(2)
    w = r.want
    assert w[1]["counters"]["n_maxlen_rejected"] == 3 + 2 + 3 + 0 and w[2]["counters"]["n_maxlen_rejected"] == 1
    assert w[1]["confirms"] == {(1, 1): ("nack", 5, True), (2, 1): ("nack", 3, True), (3, 1): ("nack", 7, True),
                                (4, 1): ("ack", 5, True)}
    assert w[2]["confirms"] == {(4, 1): ("nack", 6, False)}
    assert w[1]["bytes"] == {0: 200, 1: OVERSIZE, 2: 201, 3: 199 + OVERSIZE}
    return r


TILE_CASES = (("ta", 150, 70), ("tb", 200, 130), ("tc", SORT_TILE + 76, SORT_TILE + 6))   # queue, pairs, K


def sc_reject_tiles(dp, on=True):
    """Three reject-publish queues whose pairs of one step cross wave iterations and a sort tile:
    150 pairs with K = 70 (the second 64-pair iteration), 200 with K = 130 (the third), 1100 with
    K = 1030 (past the first tile), published interleaved with the pairs of two unlimited queues
    whose slots lie on either side.  Bodies of 3 bytes and B = 3 K - 2: pair r passes iff
    3 r < B, so exactly K pass."""
    r = BRec(dp, on)
    r.queue("ua")
    for q, _, K in TILE_CASES:
        r.queue(q, B=3 * K - 2, mode="reject-publish")
    r.queue("ub")
    r.open(1, confirm=True)
    r.open(2, confirm=True)
    for i in range(max(n for _, n, _ in TILE_CASES)):
        for q, n, _ in TILE_CASES:
            if i < n:
                r.pub(1, 1, [3], q)
        if i % 5 == 0:
            r.pub(2, 1, [7], "ua" if i % 2 else "ub")
    r.end()
    w = r.want[0]
    assert w["counters"]["n_maxlen_rejected"] == sum(n - K for _, n, K in TILE_CASES) and w["counters"]["n_ring_full"] == 0
    assert w["depth"] == {0: 110, 1: 70, 2: 130, 3: SORT_TILE + 6, 4: 110}
    assert w["confirms"] == {(1, 1): ("nack", 1450, True), (2, 1): ("ack", 220, True)}
    for i, q in enumerate(("ua", "ta", "tb", "tc", "ub")):
        r.consume(3, 1 + i, q, later=True)
    r.end(6)   # (a channel's window takes 256 deliveries a step)
    assert r.want[-1]["depth"] == dict.fromkeys(range(5), 0)
    return r


def sc_reject_fanout(dp, on=True):
    """A fanout to a reject-publish queue that refuses by bytes and to an unlimited one: the
    unlimited queue gets every message, the refusals release their references."""
    r = BRec(dp, on)
    r.queue("fb", B=25, mode="reject-publish")
    r.queue("fu")
    r.bind_fanout("fb")
    r.bind_fanout("fu")
    r.open(1, confirm=True)
    r.pub(1, 1, [10] * 6, exchange="amq.fanout")   # 0, 10, 20 pass; 30 does not
    r.end()
    r.pub(1, 1, [10] * 3, exchange="amq.fanout")
    r.consume(2, 1, "fb", later=True)
    r.consume(2, 2, "fu", later=True)
    r.end(3)
    w = r.want
    assert [x["counters"]["n_maxlen_rejected"] for x in w[:2]] == [3, 3] and w[1]["confirms"] == {(1, 1): ("nack", 9, True)}
    assert len(w[1]["events"][(2, 1)]) == 3 and len(w[1]["events"][(2, 2)]) == 9
    return r


def sc_reject_vs_ring(dp, on=True):
    """Rings that cannot grow against K.  re: a 16-slot ring holding 8, K = 8 -- exactly the
    ring's room: the refusals are the limit's.  rl: a 16-slot ring holding 12, K = 8: the ring
    ends first and every refusal is the ring's."""
    r = BRec(dp, on)
    r.queue("re", B=160, mode="reject-publish", cap=16)
    r.queue("rl", B=200, mode="reject-publish", cap=16)
    r.open(1, confirm=True)
    r.pub(1, 1, [10] * 8, "re")
    r.pub(1, 1, [10] * 12, "rl")
    r.end()
    r.pub(1, 1, [10] * 12, "re")   # Y = 80: pairs 0 .. 7 pass (80 + 70 < 160), the ring has room for 8
    r.pub(1, 1, [10] * 12, "rl")   # Y = 120: pairs 0 .. 7 pass, the ring has room for 4
    r.end()
    w = r.want
    assert (w[1]["counters"]["n_maxlen_rejected"], w[1]["counters"]["n_ring_full"]) == (4, 8)
    assert w[1]["depth"] == {0: 16, 1: 16}
    r.consume(2, 1, "re", later=True)
    r.consume(2, 2, "rl", later=True)
    r.end(2)
    return r


GROW_PAIRS = 100


def sc_reject_no_growth(dp, on=True):
    """A 16-slot ring that may grow, B = 100, 100 pairs of 10 in one step: K = 10, the ring is
    not grown for the 90 that K refuses."""
    r = BRec(dp, on)
    r.queue("rg", B=100, mode="reject-publish", keep=16)
    r.open(1, confirm=True)
    r.pub(1, 1, [10] * GROW_PAIRS, "rg")
    r.end()
    r.consume(2, 1, "rg", later=True)
    r.end(2)
    assert r.want[0]["counters"]["n_maxlen_rejected"] == GROW_PAIRS - 10 and r.want[0]["counters"]["n_ring_full"] == 0
    return r


def sc_requeue_over(dp, on=True):
    """Nack-requeue puts the bytes above B.  qj (reject-publish, B = 30): 3 x 10 delivered, 3 more
    accepted, the requeue makes 60 > B -- accepted; the step's and the next step's publishes are
    all refused.  qd (drop-head, B = 30), the consumer's flow off: the requeued oldest three are
    trimmed."""
    r = BRec(dp, on)
    r.open(1, confirm=True)
    r.open(4, confirm=True)
    r.queue("qj", B=30, mode="reject-publish")
    r.queue("qd", B=30)
    for q, conn in (("qj", 2), ("qd", 3)):
        r.consume(conn, 1, q, no_ack=False, prefetch=3)
    r.pub(1, 1, [10] * 3, "qj")
    r.pub(4, 1, [10] * 3, "qd")
    r.end()
    r.pub(1, 1, [10] * 3, "qj")
    r.pub(4, 1, [10] * 3, "qd")
    r.end()
    r.nack_all(2, 1)
    r.nack_all(3, 1)
    r.flow(2, 1, False)
    r.flow(3, 1, False)
    r.pub(1, 1, [10] * 2, "qj")
    r.end()
    r.pub(1, 1, [0, 10], "qj")
    r.end()
    r.flow(2, 1, True)
    r.flow(3, 1, True)
    r.end()
    for _ in range(3):
        r.ack_all(2, 1)
        r.ack_all(3, 1)
        r.end()
    w = r.want
    assert [x["counters"]["n_maxlen_rejected"] for x in w[:4]] == [0, 0, 2, 2]
    assert w[2]["counters"]["n_maxlen_dropped"] == 3 and w[2]["bytes"] == {0: 60, 1: 30}
    assert [(e[2], e[3]) for e in w[4]["events"][(2, 1)]] == [(sized("qj", i, 10), True) for i in range(3)]
    assert [(e[2], e[3]) for e in w[4]["events"][(3, 1)]] == [(sized("qd", i, 10), False) for i in (3, 4, 5)]
    return r


EXIT_STEP_MS = 600
EXIT_QMAX = 8


def sc_exits(dp, on=True):
    """Every way out of the ready list takes its bytes along: TTL expiry, Basic.Get in a step
    and between steps, a purge and the step after it, a delete with a redeclare of the slot, and
    the dispatch to a consumer with prefetch.  No limit binds (B is large): the ready bytes are
    the device's bookkeeping alone, on limited and unlimited queues."""
    r = BRec(dp, on, EXIT_STEP_MS)
    r.queue("xt", ttl=1000)                      # TTL expiry
    r.queue("xg", B=1 << 20)                     # Gets
    r.queue("xp", B=1 << 20, mode="reject-publish")   # purge
    r.queue("xd")                                # delete and redeclare
    r.queue("xc", B=1 << 20)                     # prefetch consumer
    r.open(1)
    r.open(3)
    r.open(4)
    r.consume(2, 1, "xc", no_ack=False, prefetch=2)
    r.pub(1, 1, [11, 12, 13], "xt")
    r.pub(1, 1, [21, 22, 23, 24], "xg")
    r.pub(1, 1, [31, 32], "xp")
    r.pub(1, 1, [41, 42], "xd")
    r.pub(1, 1, [51, 52, 53, 54, 55], "xc")
    r.end()
    assert r.want[0]["bytes"] == {0: 36, 1: 90, 2: 63, 3: 83, 4: 53 + 54 + 55}
    r.get(3, 1, "xg")                            # in the step: 21 leaves
    r.pub(1, 1, [14], "xt")
    r.end()
    r.get_between(4, 1, "xg")                    # between steps: 22 leaves
    r.purge("xp")
    # freed slots are reused last: with the narrow table (q_max = 8) three fillers take the slots
    # never used and the redeclare gets the deleted queue's slot, stale bytes and all; with the
    # wide one it gets a fresh slot
    slot = r.delete("xd")
    if dp.q_max == EXIT_QMAX:
        for i in range(5, EXIT_QMAX):
            r.queue(f"xf{i}", later=True, slot=i)
    else:
        slot = 5
    r.queue("xn", B=1 << 20, later=True, slot=slot)
    r.ack_all(2, 1)
    r.pub(1, 1, [5], "xn")
    r.end()                                      # (1200 ms: the first three of xt expire)
    assert {s: b for s, b in r.want[2]["bytes"].items() if b} == {0: 14, 1: 23 + 24, slot: 5, 4: 55}
    assert r.want[2]["counters"]["n_expired"] == 3 + 2
    r.ack_all(2, 1)
    r.consume(5, 1, "xg", later=True)
    r.consume(5, 2, "xn", later=True)
    r.end(3)
    return r


def sc_wide_limit(dp, on=True):
    """B = 2^32 + 5 must not behave as 5: a few small messages, nothing refused or trimmed."""
    r = BRec(dp, on)
    r.queue("wj", B=(1 << 32) + 5, mode="reject-publish")
    r.queue("wd", B=(1 << 32) + 5)
    r.open(1, confirm=True)
    r.pub(1, 1, [3, 3, 3, 3], "wj")
    r.pub(1, 1, [3, 3, 3, 3], "wd")
    r.end()
    r.pub(1, 1, [3, 3], "wj")
    r.pub(1, 1, [3, 3], "wd")
    r.end()
    r.consume(2, 1, "wj", later=True)
    r.consume(2, 2, "wd", later=True)
    r.end(2)
    assert all(not any(w["counters"][c] for c in ("n_maxlen_dropped", "n_maxlen_rejected")) for w in r.want)
    assert r.want[1]["depth"] == {0: 6, 1: 6} and r.want[1]["confirms"] == {(1, 1): ("ack", 12, True)}
    return r


DURABLE_B = 500
DURABLE_N = 2600


def sc_durable_budget(dp, on=True):
    """A persisting plane, one durable drop-head queue with B = 500, persistent bodies of 10.  The
    byte trim draws on the TTL walk's record budget (20 reservations of 64 a step here, of which
    the walk's look at the head takes one), so 2600 arrivals are trimmed over three steps (1216,
    1216, 118); then the queue holds 50 entries of 500 bytes and stays."""
    r = BRec(dp, on)
    assert persists(dp) and (persist_max(dp) >> 2) == 1280
    r.persist_budget = (persist_max(dp) >> 2) // 64
    r.queue("db", B=DURABLE_B, durable=True)
    r.open(1)
    r.pub(1, 1, [10] * DURABLE_N, "db", props=PERSISTENT)
    r.end(5)
    r.consume(2, 1, "db", later=True)
    r.end(2)
    assert [w["counters"]["n_maxlen_dropped"] for w in r.want[:5]] == [1216, 1216, 118, 0, 0]
    assert [(w["depth"][0], w["bytes"][0]) for w in r.want[2:5]] == [(50, DURABLE_B)] * 3
    return r


DL_CFG = dict(dead_letter=True, dead_max=1024, dead_bytes=1 << 20)
XD_CFG = dict(DL_CFG, x_death=True)


def sc_dead_letter_bytes(dp, on=True):
    """A drop-head queue with B = 50 and a dead-letter exchange: the byte-trimmed entries arrive
    at the exchange's queue in the next step, in order: 7 of 12 bodies of 10, then, when two of 30
    arrive, the other five and the first 30 (60 is still above B)."""
    r = BRec(dp, on)
    r.queue("dq")
    r.bind_fanout("dq")
    r.queue("ds", B=50, dlq="dq")
    r.open(1)
    r.pub(1, 1, [10] * 12, "ds")
    r.end()
    r.pub(1, 1, [30, 30], "ds")
    r.end()
    r.consume(2, 1, "dq", later=True)
    r.consume(2, 2, "ds", later=True)
    r.end(3)
    w = r.want
    assert [x["counters"]["n_maxlen_dropped"] for x in w[:2]] == [7, 6] and w[1]["depth"] == {0: 7, 1: 1}
    assert [e[2] for e in w[2]["events"][(2, 1)]] == r.died and len(r.died) == 13
    return r


def sc_off(dp, on=False):
    """``queue_limits`` on, the byte flag off: queues declared with the byte keyword behave as
    queues without it (the count limit of the third still holds)."""
    r = BRec(dp, False)
    r.queue("od", B=5)
    r.queue("oj", B=5, mode="reject-publish")
    r.queue("oc", L=2, B=5)
    r.open(1, confirm=True)
    for q in ("od", "oj", "oc"):
        r.pub(1, 1, [10] * 6, q)
    r.end()
    for i, q in enumerate(("od", "oj", "oc")):
        r.consume(2, 1 + i, q, later=True)
    r.end(2)
    assert r.want[0]["confirms"] == {(1, 1): ("ack", 18, True)} and r.want[0]["depth"] == {0: 6, 1: 6, 2: 2}
    assert r.want[0]["counters"]["n_maxlen_dropped"] == 4 and not r.want[0]["counters"]["n_maxlen_rejected"]
    return r


SCENARIOS = {
    "trim_wave_edges": Scenario(sc_trim_wave_edges, {}, 0, True),
    "trim_sizes": Scenario(sc_trim_sizes, {}, 0, True),
    "both_limits": Scenario(sc_both_limits, {}, 0, True),
    "reject_prefix": Scenario(sc_reject_prefix, {}, 0, True),
    "reject_tiles": Scenario(sc_reject_tiles, dict(pair_max=4096), 0, True),
    "reject_fanout": Scenario(sc_reject_fanout, {}, 0, True),
    "reject_vs_ring": Scenario(sc_reject_vs_ring, {}, 0, True),
    "reject_no_growth": Scenario(sc_reject_no_growth, {}, 0, True),
    "requeue_over": Scenario(sc_requeue_over, {}, 0, True),
    "exits": Scenario(sc_exits, dict(q_max=EXIT_QMAX), EXIT_STEP_MS, False),
    "wide_limit": Scenario(sc_wide_limit, {}, 0, True),
    "durable_budget": Scenario(sc_durable_budget, DURABLE_CFG, 0, True),
    "dead_letter_bytes": Scenario(sc_dead_letter_bytes, DL_CFG, 0, True),
    "dead_letter_bytes_x_death": Scenario(sc_dead_letter_bytes, XD_CFG, 0, True),
}
# the two key widths TWO_PASS stands for: every scenario again with q_max = 4096
WIDTHS = {"narrow": {}, "wide": TWO_PASS}
OFF = Scenario(sc_off, {}, 0, True)


def x_death_reasons(outs, conn, ch):
    """The x-death[0].reason of every delivery on (conn, ch), from the property bytes on the wire."""
    from chanamq_amd.protocol.codec import FrameParser, decode_content_header
    out = []
    for o in outs:
        fp = FrameParser()
        for fr in fp.feed(o["egress"].get(conn, b"")):
            if fr.type == 2 and fr.channel == ch:
                out.append(decode_content_header(fr.payload)[2]["headers"]["x-death"][0]["reason"])
    return out


# ================================================================ sharded
# a drop-head and a reject-publish queue with byte limits owned by rank 1, published from rank 0 on
# a confirm channel: the owner trims / refuses, the publisher gets Basic.Ack
SHARD_STEPS, SHARD_N, SHARD_SIZE = 6, 8, 10
SHARD_QUEUES = (("bd", 30, "drop-head"), ("bj", 15, "reject-publish"))
PUB_CONN, CONS_CONN = 1, 10


def sharded_cluster(cfg, lag=0, gpu=False, graph=True):
    from chanamq_amd.parallel.cluster import LocalCluster
    from xchg_scenarios import golden_kw
    kw = dict(queue_limits=True, queue_limit_bytes=True)
    if gpu:
        import torch

        from chanamq_amd.engine.dataplane import GpuDataPlane
        torch.cuda.set_device(0)
        return LocalCluster(lambda **k: GpuDataPlane(graph=graph, exchange_lag=lag, **kw, **cfg, **k), 2)
    from chanamq_amd.engine.golden import GoldenDataPlane
    return LocalCluster(lambda **k: GoldenDataPlane(exchange_lag=lag, **kw, **golden_kw(cfg), **k), 2)


def sharded_run(cl, now=NOW):
    """-> per rank and step (egress by connection, the two counters, the ready bytes by queue)."""
    for q, _, _ in SHARD_QUEUES:
        cl.shard_map.place(VH, q, 1)
    for p in cl.planes:
        for q, B, mode in SHARD_QUEUES:
            p.declare_queue(VH, q, capacity=64, max_length_bytes=B, overflow=mode)
    cl[0].open_connection(PUB_CONN, VH)
    cl[0].open_channel(PUB_CONN, 1)
    cl[0].confirm_select(PUB_CONN, 1)
    data = b"".join(publish_command(1, "", q, sized(q, i, SHARD_SIZE)) for q, _, _ in SHARD_QUEUES for i in range(SHARD_N))
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
            nbytes = {q: int(cl[r].queue_bytes(cl[r].queues[(VH, q)].slot)) for q, _, _ in SHARD_QUEUES} if r == 1 else {}
            outs[r].append((dict(eg), int(cnt.get("n_maxlen_dropped", 0)), int(cnt.get("n_maxlen_rejected", 0)), nbytes))
    return outs


def sharded_check(outs):
    """What the rule says, from the wire: Acks only on the publisher's rank; the newest 3 bodies
    (30 bytes) of the drop-head queue and the first 2 of the reject-publish queue (0 and 10 are
    below 15) on the owner's."""
    conf, got = [], defaultdict(list)
    for r in range(2):
        for k, (eg, _, _, _) in enumerate(outs[r]):
            ev, empty, c = observe(dict(egress=eg), k)
            conf += [(r, key, v) for key, v in c.items()]
            for key, es in ev.items():
                assert r == 1 and key == (CONS_CONN, 1)
                for e in es:
                    got[e[1]].append(e[2])
    assert conf == [(0, (PUB_CONN, 1), ("ack", 2 * SHARD_N, True))]
    assert dict(got) == {"c-bd": [sized("bd", i, SHARD_SIZE) for i in range(SHARD_N - 3, SHARD_N)],
                         "c-bj": [sized("bj", i, SHARD_SIZE) for i in range(2)]}
    assert [sum(o[1] for o in outs[r]) for r in (0, 1)] == [0, SHARD_N - 3]
    assert [sum(o[2] for o in outs[r]) for r in (0, 1)] == [0, SHARD_N - 2]
    assert outs[1][2][3] == {"bd": 30, "bj": 20} and outs[1][-1][3] == {"bd": 0, "bj": 0}
