"""Dead-lettering (x-dead-letter-exchange / x-dead-letter-routing-key, ``dead_letter=True``) in the
``limit_scenarios`` style: each scenario is ``(dp, on) -> Rec`` with its own engine overrides on
top of ``gpu_cfg.CFG``.

``Rec`` is the scenarios' own record.  It keeps a plain Python list per queue, a list of exchanges
with their bindings as predicates, and a plain list for the dead list, and applies the rules as
CHANGES.md states them: an entry of a queue with a dead-letter exchange that expires at the head,
is trimmed by x-max-length or is rejected without requeue joins the dead list (purged entries never
do; without room the walk stops and a reject is deferred); the step after, the pending items in
the order (step died, queue slot, queue position, reason, channel, tag), as far as the pass's
record and payload room goes, are published to the exchange as new messages behind the step's own
publishes.  While a scenario is written the record builds each step's wire input and predicts
every delivery (with its exchange and routing-key fields, properties and body), the depths, the
counters and, on a persisting plane, the store records.  It never looks at the golden model:
``check`` judges the golden model's run and the HIP data plane's alike.
"""

from collections import defaultdict, namedtuple

from chanamq_amd.engine.traffic import ack_frame, publish_command
from chanamq_amd.protocol.codec import FrameParser, Method, decode_content_header, decode_method, render_command
from consumer_scenarios import GOLDEN_KEYS, body_of
from dp_scenarios import NOW, VH

Scenario = namedtuple("Scenario", "fn cfg now_step_ms drained")
COUNTERS = ("n_deliv", "n_expired", "n_requeue", "n_ring_full", "n_maxlen_dropped", "n_maxlen_rejected",
            "n_dl_expired", "n_dl_maxlen", "n_dl_rejected", "n_dl_unrouted", "n_dl_dropped", "n_dl_pending")
DELIVER_CAP = 4096
PERSISTENT = {"delivery_mode": 2}
EXPIRED, MAXLEN, REJECTED = 0, 1, 2
MS_MAX = 256           # dataplane.hip: multiple settles of a channel resolved exactly per step


def a16(n):
    return (n + 15) & ~15


def words_match(pat, key):
    """Topic match over words: '*' one word, '#' any number (the few patterns used here)."""
    p, k = pat.split(b"."), key.split(b".")

    def m(i, j):
        if i == len(p):
            return j == len(k)
        if p[i] == b"#":
            return any(m(i + 1, jj) for jj in range(j, len(k) + 1))
        return j < len(k) and (p[i] == b"*" or p[i] == k[j]) and m(i + 1, j + 1)
    return m(0, 0)


class Entry:
    __slots__ = ("ex", "rk", "props", "body", "expire", "red", "seq", "psize")

    def __init__(self, ex, rk, props, body, expire, seq, psize):
        self.ex, self.rk, self.props, self.body, self.expire, self.red, self.seq = ex, rk, props, body, expire, False, seq
        self.psize = psize   # bytes of the property list on the wire


def props_size(props):
    """Bytes of the property list (flags + values) of a content header carrying ``props``."""
    frames = list(FrameParser().feed(publish_command(1, "", "", b"", props or None)))
    return len(frames[1].payload) - 12


class Rec:
    def __init__(self, dp, on=True, now_step_ms=0, dead_max=1024, dead_bytes=8 << 20, room=64, persist_budget=None):
        self.dp, self.on, self.now_step_ms = dp, on, now_step_ms
        self.dead_max, self.dead_bytes, self.room = dead_max, dead_bytes, min(room, dead_max)
        self.persist_budget = persist_budget   # (persisting plane) records the walks of durable queues may take a step
        self.q, self.x, self.chan = {}, {"": dict(type="default", binds=[], edges=[])}, {}
        self.dead = []
        self.steps, self.want = [], []
        self.seq = 0
        self.persist = persist_budget is not None
        self._new_step()

    def _new_step(self):
        self.cur = defaultdict(bytes)
        self.ops, self.pubs, self.settles = [], [], []

    # ---- topology
    def _call(self, later, name, *a, **kw):
        if later:
            self.ops.append((name, a, kw))
        else:
            getattr(self.dp, name)(*a, **kw)

    def exchange(self, name, type_="direct", later=False):
        self._call(later, "declare_exchange", VH, name, type_)
        self.x[name] = dict(type=type_, binds=[], edges=[])

    def delete_exchange(self, name):
        self.ops.append(("delete_exchange", (VH, name), {}))
        del self.x[name]

    def queue(self, name, ttl=0, L=None, dlx=None, dlk=None, durable=False, mode=None, **kw):
        extra = {}
        if dlx is not None and hasattr(self.dp, "dead_letter"):   # (the keywords exist with the feature)
            extra.update(dead_letter_exchange=dlx, **({} if dlk is None else {"dead_letter_routing_key": dlk}))
        if L is not None:
            extra.update(max_length=L, **({"overflow": mode} if mode else {}))
        slot = self.dp.declare_queue(VH, name, ttl_ms=ttl, durable=durable, **extra, **kw)
        self.q[name] = dict(slot=slot, ttl=ttl, L=L, mode=mode or "drop-head", dlx=dlx if self.on else None,
                            dlk=None if dlk is None else dlk.encode(), durable=durable, items=[], cons=None, serial=0, head=0)

    def bind(self, q, exchange, key="", args=None, pred=None):
        self.dp.bind(VH, q, exchange, key, *([args] if args is not None else []))
        self.x[exchange]["binds"].append((q, key.encode(), pred))

    def bind_x(self, dst, src, key=""):
        self.dp.bind_exchange(VH, dst, src, key)
        self.x[src]["edges"].append((dst, key.encode()))

    def open(self, conn, ch=1):
        if not any(c == conn for c, _ in self.chan):
            self.dp.open_connection(conn, VH)
        self.dp.open_channel(conn, ch)
        self.chan[(conn, ch)] = dict(tag=0, unacked=[], slot=self.dp.chslot(conn, ch))

    def consume(self, conn, ch, q, no_ack=True, prefetch=0, later=False):
        tag = "c-" + q
        if (conn, ch) not in self.chan:
            if not any(c == conn for c, _ in self.chan):
                self._call(later, "open_connection", conn, VH)
            self._call(later, "open_channel", conn, ch)
            self.chan[(conn, ch)] = dict(tag=0, unacked=[], slot=None)
        if prefetch:
            self._call(later, "qos", conn, ch, prefetch_count=prefetch)
        self._call(later, "consume", conn, ch, VH, q, tag, no_ack=no_ack)
        self.q[q]["cons"] = dict(conn=conn, ch=ch, tag=tag, no_ack=no_ack, prefetch=prefetch)

    def purge(self, q):
        self.ops.append(("purge", (self.q[q]["slot"],), {}))
        for e in self.q[q]["items"]:
            e.expire = 1

    def delete_queue(self, q):
        assert not self.q[q]["items"], "scenario: delete an empty queue (a purge and a step before)"
        self.ops.append(("delete_queue", (VH, q), {}))
        del self.q[q]
        for x in self.x.values():
            x["binds"] = [b for b in x["binds"] if b[0] != q]

    # ---- the current step
    def pub(self, conn, ch, n, q=None, exchange="", key=None, props=None, expire_ms=0, size=0, body=None):
        """n publishes: to queue ``q`` through the default exchange, or to ``exchange`` with ``key``."""
        name = q if q is not None else exchange
        rk = q if q is not None else (key or "")
        for _ in range(n):
            if q is not None:
                i, self.q[q]["serial"] = self.q[q]["serial"], self.q[q]["serial"] + 1
            else:
                i = self.seq
            b = body_of(name or "x", i, size) if body is None else body
            p = dict(props or {})
            if expire_ms:
                p["expiration"] = str(expire_ms)
            self.cur[conn] += publish_command(ch, exchange, rk, b, p or None)
            self.pubs.append((conn, len(self.pubs), exchange, rk.encode(), b, p, expire_ms))
            self.seq += 1

    def settle(self, conn, ch, kind, tag, multiple=False, requeue=False):
        """kind: ack | nack | reject, as on the wire."""
        if kind == "ack":
            self.cur[conn] += ack_frame(ch, tag, multiple=multiple)
        elif kind == "nack":
            self.cur[conn] += render_command(ch, Method("basic.nack", delivery_tag=tag, multiple=multiple, requeue=requeue))
        else:
            assert not multiple
            self.cur[conn] += render_command(ch, Method("basic.reject", delivery_tag=tag, requeue=requeue))
        self.settles.append((conn, ch, 0 if kind == "ack" else (1 if requeue else 2), tag, multiple))

    def tx_settle(self, conn, ch, kind, tag, multiple=False, requeue=False):
        """The same mark made between steps (Tx.Commit: ``apply_ack``), before the current step."""
        self.ops.append(("apply_ack", (conn, ch, tag), dict(multiple=multiple, requeue=requeue, kind=kind)))
        self.settles.append((conn, ch, 0 if kind == "ack" else (1 if requeue else 2), tag, multiple))

    # ---- the rules
    def route(self, exchange, rk, props, seen=None):
        """Queue names the exchange (and the exchanges its edges lead to) routes the message to."""
        seen = set() if seen is None else seen
        x = self.x.get(exchange)
        if x is None or exchange in seen:
            return set()
        seen.add(exchange)

        def hit(key, pred):
            if pred is not None:
                return pred(rk, props)
            return {"default": key == rk, "direct": key == rk, "fanout": True}.get(x["type"], None) \
                if x["type"] != "topic" else words_match(key, rk)
        out = {q for q in self.q if x["type"] == "default" and q.encode() == rk}
        out |= {q for q, key, pred in x["binds"] if hit(key, pred)}
        for dst, key in x["edges"]:
            if hit(key, None):
                out |= self.route(dst, rk, props, seen)
        return out

    def _enqueue(self, qn, e, now, cnt):
        q = self.q[qn]
        if q["L"] is not None and q["mode"] == "reject-publish" and len(q["items"]) >= q["L"]:
            cnt["n_maxlen_rejected"] += 1
            return
        ne = Entry(e.ex, e.rk, e.props, e.body, e.expire, self.seq, e.psize)
        self.seq += 1
        if q["ttl"]:
            ne.expire = min(x for x in (ne.expire, now + q["ttl"]) if x)
        if q["durable"] and self.persist and e.props.get("delivery_mode") == 2:
            self.stored.append((q["slot"], q["head"] + len(q["items"]), e.ex.encode(), e.rk, e.body))
        q["items"].append(ne)

    def _leave(self, qn, e, qpos, reason, k, cnt):
        """Entry ``e`` leaves the head of ``qn`` expired or trimmed: True if it went (released, lost
        or on the dead list), False if it stays because the dead list is full."""
        q = self.q[qn]
        if q["dlx"] is not None and e.expire != 1:
            if q["dlx"] not in self.x:
                cnt["n_dl_unrouted"] += 1
            elif len(self.dead) >= self.dead_max:
                return False
            else:
                self._join(qn, e, qpos, reason, k, 0, 0, cnt)
        if q["durable"] and self.persist and e.props.get("delivery_mode") == 2:
            self.consumed.append((q["slot"], qpos, 1))
        return True

    def _join(self, qn, e, qpos, reason, k, ch, tag, cnt):
        q = self.q[qn]
        self.dead.append(dict(e=e, q=q["slot"], qpos=qpos, reason=reason, step=k, ch=ch, tag=tag, ex=q["dlx"],
                              rk=e.rk if q["dlk"] is None else q["dlk"]))
        cnt[("n_dl_expired", "n_dl_maxlen", "n_dl_rejected")[reason]] += 1

    def end(self, n=1):
        for _ in range(n):
            self._end()

    def _end(self):
        k = len(self.steps)
        now = NOW + self.now_step_ms * k
        cnt = dict.fromkeys(COUNTERS, 0)
        ev = defaultdict(list)
        self.stored, self.consumed = [], []
        # (1) the step's own publishes, in publish order (connection, then wire order)
        for conn, _, ex, rk, body, props, exp_ms in sorted(self.pubs, key=lambda p: p[:2]):
            e = Entry(ex, rk, props, body, now + exp_ms if exp_ms else 0, 0, props_size(props))
            for qn in sorted(self.route(ex, rk, props), key=lambda n: self.q[n]["slot"]):
                self._enqueue(qn, e, now, cnt)
        # (2) the dead pass: the pending items in their order, the prefix that fits, behind (1)
        self.dead.sort(key=lambda d: (d["step"], d["q"], d["qpos"], d["reason"], d["ch"], d["tag"]))
        take = nrec = nbytes = 0
        for d in self.dead:
            d["size"] = a16(a16(len(d["ex"].encode()) + len(d["rk"]) + d["e"].psize) + len(d["e"].body))
            if d["size"] <= self.dead_bytes:
                if nrec >= self.room or nbytes + d["size"] > self.dead_bytes:
                    break
                nrec, nbytes = nrec + 1, nbytes + d["size"]
            take += 1
        taken, self.dead = self.dead[:take], self.dead[take:]
        for d in taken:
            if d["size"] > self.dead_bytes:
                cnt["n_dl_dropped"] += 1
                continue
            qs = self.route(d["ex"], d["rk"], d["e"].props) if d["ex"] in self.x else set()
            if not qs:
                cnt["n_dl_unrouted"] += 1
            e = Entry(d["ex"], d["rk"], d["e"].props, d["e"].body, 0, 0, d["e"].psize)
            for qn in sorted(qs, key=lambda n: self.q[n]["slot"]):
                self._enqueue(qn, e, now, cnt)
        # (3) settles: single marks first, then the multiple ones in wire order (the first cover
        # wins); acks release, requeues go back in front of the heads, rejects without requeue are
        # dead-lettered where the queue has a dead-letter exchange (all of a channel's, or -- the
        # list full -- none: the marks stay for the next step), else they are acks
        back = defaultdict(list)
        for key in sorted(self.chan):
            c = self.chan[key]
            mine = [s for s in self.settles if s[:2] == key]
            assert len(c["unacked"]) <= 256 or self.dead_max - len(self.dead) >= len(c["unacked"]), \
                "scenario: one 256-tag chunk per channel where the list's room may bind"
            for _, _, kind, tag, multiple in mine:
                if not multiple:
                    for u in c["unacked"]:
                        if u["tag"] == tag and u["mark"] is None:
                            u["mark"] = kind
            top = 0
            for _, _, kind, tag, multiple in mine:
                if multiple:
                    tag = tag or c["tag"]
                    if tag > top:
                        for u in c["unacked"]:
                            if top < u["tag"] <= tag and u["mark"] is None:
                                u["mark"] = kind
                        top = tag
            if not self.on:
                for u in c["unacked"]:
                    u["mark"] = 0 if u["mark"] == 2 else u["mark"]

            def dlq(u):
                return u["mark"] == 2 and u["q"] in self.q and self.q[u["q"]]["dlx"] in self.x
            if sum(1 for u in c["unacked"] if dlq(u)) > self.dead_max - len(self.dead):
                continue   # deferred
            for u in c["unacked"]:
                if u["mark"] is None:
                    continue
                q = self.q.get(u["q"])
                rec = q is not None and q["durable"] and self.persist and u["e"].props.get("delivery_mode") == 2
                if u["mark"] == 1:
                    back[u["q"]].append(u["e"])
                    cnt["n_requeue"] += 1
                    if rec:
                        self.consumed.append((q["slot"], u["qpos"], 4))
                    continue
                if u["mark"] == 2 and q is not None and q["dlx"] is not None:
                    if dlq(u):
                        self._join(u["q"], u["e"], u["qpos"], REJECTED, k, c["slot"], u["tag"], cnt)
                    else:
                        cnt["n_dl_unrouted"] += 1
                if rec:
                    self.consumed.append((q["slot"], u["qpos"], 0))
            c["unacked"] = [u for u in c["unacked"] if u["mark"] is None]
        for qn, es in back.items():
            for e in es:
                e.red = True
            self.q[qn]["items"][:0] = sorted(es, key=lambda e: e.seq)
            self.q[qn]["head"] -= len(es)
        # (4) per queue, in slot order: TTL walk, dispatch, trim
        budget = self.persist_budget
        for qn, q in sorted(self.q.items(), key=lambda kv: kv[1]["slot"]):
            items = q["items"]
            n_it = 0
            while items:
                if q["durable"] and self.persist and n_it % 64 == 0:   # 64 records reserved an iteration
                    if budget < 64:
                        break
                    budget -= 64
                if not (items[0].expire and items[0].expire <= now):
                    break
                if not self._leave(qn, items[0], q["head"], EXPIRED, k, cnt):
                    break
                items.pop(0)
                q["head"] += 1
                cnt["n_expired"] += 1
                n_it += 1
            c = q["cons"]
            if c is not None and items:
                chan = self.chan[(c["conn"], c["ch"])]
                g = min(len(items), DELIVER_CAP)
                if not c["no_ack"] and c["prefetch"]:
                    g = min(g, max(c["prefetch"] - sum(1 for u in chan["unacked"] if u["q"] == qn), 0))
                for i, e in enumerate(items[:g]):
                    chan["tag"] += 1
                    rec = q["durable"] and self.persist and e.props.get("delivery_mode") == 2
                    if not c["no_ack"]:
                        chan["unacked"].append(dict(tag=chan["tag"], q=qn, e=e, qpos=q["head"] + i, mark=None))
                        if rec:
                            self.consumed.append((q["slot"], q["head"] + i, 3))
                    elif rec:
                        self.consumed.append((q["slot"], q["head"] + i, 0))
                    ev[(c["conn"], c["ch"])].append((c["tag"], e.ex, e.rk, e.props, e.body, e.red, chan["tag"]))
                    cnt["n_deliv"] += 1
                del items[:g]
                q["head"] += g
            if q["L"] is not None and q["mode"] == "drop-head":
                n_it = 0
                while len(items) > q["L"]:
                    if q["durable"] and self.persist and n_it % 64 == 0:
                        if budget < 64:
                            break
                        budget -= 64
                    if not self._leave(qn, items[0], q["head"], MAXLEN, k, cnt):
                        break
                    items.pop(0)
                    q["head"] += 1
                    cnt["n_maxlen_dropped"] += 1
                    n_it += 1
        cnt["n_dl_pending"] = len(self.dead)
        inp = {c: b for c, b in self.cur.items()}
        if self.ops:
            inp["__ops__"] = self.ops
        self.steps.append(inp)
        w = dict(events=dict(ev), counters=cnt, depth={q["slot"]: len(q["items"]) for q in self.q.values()})
        if self.persist:
            w["consumed"], w["stored"] = sorted(self.consumed), sorted(self.stored)
        self.want.append(w)
        self._new_step()


# ---------------------------------------------------------------- planes and runner
def cfg_of(sc, base):
    return dict(base, **sc.cfg)


DL_KEYS = ("dead_max", "dead_bytes", "restore_max")


def golden_plane(cfg, on=True):
    from chanamq_amd.engine.golden import GoldenDataPlane
    kw = {k: cfg[k] for k in GOLDEN_KEYS + ("ring_pool", "deliv_max", "egress_cap", "persist_max") if k in cfg}
    if cfg.get("persist"):
        kw["persist"] = True
    for k in ("queue_limits", "headers_match"):
        if cfg.get(k):
            kw[k] = True
    if on:
        kw.update(dead_letter=True, **{k: cfg[k] for k in DL_KEYS if k in cfg})
    return GoldenDataPlane(**kw)


def gpu_plane(cfg, graph, on=True):
    from chanamq_amd.engine.dataplane import GpuDataPlane
    cfg = dict(cfg)
    if not on:
        for k in DL_KEYS[:2]:
            cfg.pop(k, None)
    return GpuDataPlane(graph=graph, **(dict(cfg, dead_letter=True) if on else cfg))


def persists(dp):
    return bool(dp.info.get("persist")) if hasattr(dp, "eng") else bool(dp.persist)


def run_dlx(dp, rec):
    """Drive dp through the record's steps (control ops first, the clock advanced per step)."""
    outs = []
    for k, inp in enumerate(rec.steps):
        inp = dict(inp)
        for op in inp.pop("__ops__", []):
            getattr(dp, op[0])(*op[1], **op[2])
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
            o["stored"] = sorted((int(p[2]), int(p[3]), bytes(p[5]), bytes(p[6]), bytes(p[8])) for p in dp.take_persist())
            o["consumed"] = sorted((int(q), int(qpos), int(kind)) for _, q, qpos, kind in dp.take_consumed())
        outs.append(o)
    return outs


def observe(out, k):
    """One step's deliveries as the record states them: {(conn, ch): [(consumer tag, exchange,
    routing key, properties, body, redelivered, delivery tag)]}; anything else on the wire fails."""
    ev = defaultdict(list)
    for conn in sorted(out["egress"]):
        fp, cur = FrameParser(), None
        for fr in fp.feed(out["egress"][conn]):
            if fr.type == 1:
                assert cur is None, f"step {k} conn {conn}: method frame inside content"
                m = decode_method(fr.payload)
                assert m.name == "basic.deliver", f"step {k} conn {conn}: unexpected {m.name}"
                cur = [fr.channel, m, None, [], None]
                continue
            assert cur is not None and fr.channel == cur[0], f"step {k} conn {conn}: stray content frame"
            if fr.type == 2:
                _, cur[2], cur[4] = decode_content_header(fr.payload)
            else:
                cur[3].append(fr.payload)
            if cur[2] is not None and sum(map(len, cur[3])) >= cur[2]:
                m = cur[1]
                rk = m.routing_key if isinstance(m.routing_key, bytes) else m.routing_key.encode()
                ev[(conn, cur[0])].append((m.consumer_tag, m.exchange, rk, {a: b for a, b in cur[4].items() if b is not None},
                                           b"".join(cur[3]), bool(m.redelivered), m.delivery_tag))
                cur = None
        assert cur is None and not fp.buf, f"step {k} conn {conn}: egress ends inside a command"
    return dict(ev)


def check(rec, outs):
    """The run against the record, step by step."""
    assert len(outs) == len(rec.want)
    for k, (o, w) in enumerate(zip(outs, rec.want)):
        ev = observe(o, k)
        brief = lambda d: {c: [(e[1], e[2], e[4][:24], e[5]) for e in v] for c, v in d.items()}   # noqa: E731
        assert ev == w["events"], f"step {k}: deliveries differ: got {brief(ev)}, expected {brief(w['events'])}"
        assert o["counters"] == w["counters"], f"step {k}: counters {o['counters']}, expected {w['counters']}"
        assert o["depth"] == w["depth"], f"step {k}: depths {o['depth']}, expected {w['depth']}"
        if "consumed" in w:
            assert o["consumed"] == w["consumed"], f"step {k}: consumed records {o['consumed']}, expected {w['consumed']}"
            assert o["stored"] == w["stored"], f"step {k}: persist records differ"


def bodies(w, key):
    return [e[4] for e in w["events"].get(key, [])]


# ---------------------------------------------------------------- scenarios
TTL_STEP = 600   # ms a step; a 1000 ms TTL expires in the second step after the publish


def sc_ttl_edges(dp, on=True):
    """63, 64 and 65 expired entries at three heads (a wave less one, a wave, a wave and one of the
    64-entry walk), behind each one live entry; a queue TTL and per-message expirations mixed.
    Every dead letter reaches the parking queue once, in (queue slot, position) order, with the
    dead-letter exchange and its own key in the Deliver; the live entries stay."""
    r = Rec(dp, on, TTL_STEP, room=64)
    r.exchange("dlx", "fanout")
    r.queue("park")
    r.bind("park", "dlx")
    for n in (63, 64, 65):
        r.queue(f"t{n}", dlx="dlx", ttl=1000 if n == 64 else 0)
    r.open(1)
    for n in (63, 64, 65):
        # (the 64-queue by its x-message-ttl, every other entry also by a shorter expiration of its own)
        for i in range(n):
            r.pub(1, 1, 1, f"t{n}", expire_ms=(900 if i % 2 else 0) if n == 64 else 1000)
    r.end(2)
    for n in (63, 65):
        r.pub(1, 1, 1, f"t{n}")   # live entries behind the expired ones (the 64-queue's expires later)
    r.pub(1, 1, 1, "t64", expire_ms=0)
    r.end()
    r.consume(2, 1, "park", later=True)
    r.end(4)
    w = r.want
    if on:
        assert w[2]["counters"]["n_dl_expired"] == 192 and w[2]["counters"]["n_dl_pending"] == 192
        assert w[3]["counters"]["n_dl_pending"] == 128   # 64 records a pass
        got = sum((bodies(x, (2, 1)) for x in w), [])
        assert got[:192] == [body_of(f"t{n}", i) for n in (63, 64, 65) for i in range(n)]
        assert all(e[1] == "dlx" for x in w for e in x["events"].get((2, 1), []))
        assert w[3]["events"][(2, 1)][0][2] == b"t63"
    return r


def sc_trim(dp, on=True):
    """L = 2 with 70 arrivals in one step (two iterations of the trim: 64 and 4) and L = 0: what is
    trimmed is dead-lettered with x-dead-letter-routing-key to a direct exchange."""
    r = Rec(dp, on, room=64)
    r.exchange("dlx", "direct")
    r.queue("park")
    r.bind("park", "dlx", "trimmed")
    r.queue("l2", L=2, dlx="dlx", dlk="trimmed")
    r.queue("l0", L=0, dlx="dlx", dlk="trimmed")
    r.open(1)
    r.pub(1, 1, 70, "l2")
    r.pub(1, 1, 3, "l0")
    r.end()
    r.consume(2, 1, "park", later=True)
    r.end(3)
    w = r.want
    if on:
        assert w[0]["counters"]["n_dl_maxlen"] == 71 and w[0]["depth"][r.q["l2"]["slot"]] == 2
        assert bodies(w[1], (2, 1)) == [body_of("l2", i) for i in range(64)]
        assert bodies(w[2], (2, 1)) == [body_of("l2", i) for i in range(64, 68)] + [body_of("l0", i) for i in range(3)]
        assert all(e[1:3] == ("dlx", b"trimmed") for e in w[1]["events"][(2, 1)])
    return r


def sc_rejects(dp, on=True):
    """A single reject; Nack(multiple, requeue = 0) over three tags; ack, requeue and dead
    interleaved in one step's multiple settles of one channel; a reject on a queue without a
    dead-letter exchange, which stays an ack; a reject made between steps (Tx.Commit)."""
    r = Rec(dp, on)
    r.exchange("dlx", "fanout")
    r.queue("park")
    r.bind("park", "dlx")
    r.queue("work", dlx="dlx")
    r.queue("plain")
    r.open(1)
    r.consume(2, 1, "work", no_ack=False)
    r.consume(3, 1, "plain", no_ack=False)
    r.consume(4, 1, "park")
    r.pub(1, 1, 12, "work")
    r.pub(1, 1, 2, "plain")
    r.end()                                           # tags 1..12 on (2, 1), 1..2 on (3, 1)
    r.settle(2, 1, "reject", 1)
    r.settle(3, 1, "reject", 1)                       # no dead-letter exchange: an ack
    r.settle(3, 1, "nack", 2, multiple=True)
    r.end()
    r.settle(2, 1, "nack", 4, multiple=True)          # 2..4 dead
    r.end()
    r.settle(2, 1, "ack", 6, multiple=True)           # 5, 6 acked
    r.settle(2, 1, "nack", 8, multiple=True, requeue=True)   # 7, 8 requeued (and delivered again: 13, 14)
    r.settle(2, 1, "nack", 10, multiple=True)         # 9, 10 dead
    r.end()
    r.tx_settle(2, 1, "reject", 11)                   # between steps
    r.tx_settle(2, 1, "nack", 12, multiple=True)
    r.end()
    r.settle(2, 1, "ack", 0, multiple=True)
    r.end(2)
    w = r.want
    if on:
        assert [x["counters"]["n_dl_rejected"] for x in w[:5]] == [0, 1, 3, 2, 2]
        assert bodies(w[2], (4, 1)) == [body_of("work", 0)]
        assert bodies(w[3], (4, 1)) == [body_of("work", i) for i in (1, 2, 3)]
        assert bodies(w[4], (4, 1)) == [body_of("work", i) for i in (8, 9)]
        assert [(e[4], e[5]) for e in w[3]["events"][(2, 1)]] == [(body_of("work", i), True) for i in (6, 7)]
    else:
        assert all(not bodies(x, (4, 1)) for x in w)
    return r


def sc_reject_fold(dp, on=True):
    """MS_MAX + 2 multiple settles of one channel in one step, all Nack(requeue = 0) with rising
    tags: the two past MS_MAX are folded to their largest cover, which is dead like the rest."""
    n = MS_MAX + 2
    r = Rec(dp, on, room=64)
    r.exchange("dlx", "fanout")
    r.queue("park")
    r.bind("park", "dlx")
    r.queue("work", dlx="dlx", capacity=1024)
    r.open(1)
    r.consume(2, 1, "work", no_ack=False)
    r.pub(1, 1, n, "work")
    r.end()
    for t in range(1, n + 1):
        r.settle(2, 1, "nack", t, multiple=True)
    r.end()
    r.consume(4, 1, "park", later=True)
    r.end(6)
    if on:
        assert r.want[1]["counters"]["n_dl_rejected"] == n
        assert sum((bodies(x, (4, 1)) for x in r.want), []) == [body_of("work", i) for i in range(n)]
    return r


LIST_MAX = 64


REC = 48   # record bytes of these scenarios' messages: 16 (exchange name, key, property list) + a 30-byte body


def sc_list_limits(dp, on=True, extra=0):
    """dead_max = 64 and a dead_bytes that holds exactly 10 records.  40 entries of queues a and b
    expire in one step; the next pass takes 10, and in that step one reject and 32 / 33 / 34
    expired entries of queue c arrive -- 63, 64 and 65 for a list of 64, from two queues and one
    channel.  The reject (k_chan_advance runs first) joins, c's walk stops where the list is full,
    nothing is lost and the parking queue's order is the record's."""
    n_c = 33 + extra
    r = Rec(dp, on, TTL_STEP, dead_max=LIST_MAX, dead_bytes=10 * REC, room=64)
    r.exchange("dlx", "fanout")
    r.queue("park")
    r.bind("park", "dlx")
    for q in "abcw":
        r.queue(q, dlx="dlx")
    r.open(1)
    r.consume(3, 1, "w", no_ack=False)
    r.pub(1, 1, 30, "a", expire_ms=1000, size=30)
    r.pub(1, 1, 10, "b", expire_ms=1000, size=30)
    r.pub(1, 1, 1, "w", size=30)
    r.end(2)
    r.pub(1, 1, n_c, "c", expire_ms=400, size=30)
    r.end()                                           # a's and b's die: 40 pending
    r.settle(3, 1, "reject", 1)
    r.end()                                           # 10 taken, the reject joins, then c's
    r.consume(2, 1, "park", later=True)
    r.end(9)
    w = r.want
    if on:
        assert w[2]["counters"]["n_dl_pending"] == 40 and w[3]["counters"]["n_dl_pending"] == min(64, 64 + extra)
        assert w[3]["counters"]["n_dl_rejected"] == 1 and w[3]["counters"]["n_dl_expired"] == min(n_c, 33)
        got = sum((bodies(x, (2, 1)) for x in w), [])
        assert len(got) == 41 + n_c and len(set(got)) == len(got)
        assert [b for b in got if b.startswith(b"c:")] == [body_of("c", i, 30) for i in range(n_c)]
    return r


def sc_reject_deferred(dp, on=True):
    """The list (16 items here) full when three rejects arrive, and a pass that takes two records a
    step: the chunk's rejects join all or nothing, so the marks stay in the window slots and the
    channel stays dirty while the expired entries still queued fill what each pass frees; then
    they are dead-lettered -- nothing is lost."""
    r = Rec(dp, on, TTL_STEP, dead_max=16, dead_bytes=2 * REC, room=64)
    r.exchange("dlx", "fanout")
    r.queue("park")
    r.bind("park", "dlx")
    r.queue("a", dlx="dlx")
    r.queue("w", dlx="dlx")
    r.open(1)
    r.consume(3, 1, "w", no_ack=False)
    r.pub(1, 1, 20, "a", expire_ms=1000, size=30)
    r.pub(1, 1, 3, "w", size=30)
    r.end(3)                                          # 16 of a's join, 4 stay queued
    r.settle(3, 1, "reject", 1)
    r.settle(3, 1, "nack", 3, multiple=True)
    r.end()                                           # 2 taken: room 2 < 3 rejects
    r.consume(2, 1, "park", later=True)
    r.end(14)
    w = r.want
    if on:
        assert w[2]["counters"]["n_dl_expired"] == 16 and w[2]["depth"][r.q["a"]["slot"]] == 4
        assert w[3]["counters"]["n_dl_rejected"] == 0 and w[3]["counters"]["n_dl_pending"] == 16
        assert [x["counters"]["n_dl_rejected"] for x in w].count(3) == 1
        got = sum((bodies(x, (2, 1)) for x in w), [])
        assert sorted(got) == sorted([body_of("a", i, 30) for i in range(20)] + [body_of("w", i, 30) for i in range(3)])
    return r


def sc_payload(dp, on=True):
    """Payload exactly full and one record over -- the remainder goes a step later -- and one record
    larger than the whole buffer, which is dropped (n_dl_dropped).  dead_bytes = 4 records."""
    r = Rec(dp, on, TTL_STEP, dead_bytes=4 * REC, room=64)
    r.exchange("dlx", "fanout")
    r.queue("park")
    r.bind("park", "dlx")
    r.queue("a", dlx="dlx")
    r.open(1)
    r.consume(2, 1, "park")
    r.pub(1, 1, 4, "a", expire_ms=1000, size=30)
    r.end(3)                                          # 4 die, 4 records: exactly full
    r.pub(1, 1, 5, "a", expire_ms=1000, size=30)
    r.end(4)                                          # 5 die: 4, then 1
    r.pub(1, 1, 1, "a", expire_ms=1000, size=300)     # 320 bytes > 192
    r.pub(1, 1, 1, "a", expire_ms=1000, size=30)
    r.end(4)
    w = r.want
    if on:
        assert len(bodies(w[3], (2, 1))) == 4 and [len(bodies(w[k], (2, 1))) for k in (6, 7)] == [4, 1]
        assert sum(x["counters"]["n_dl_dropped"] for x in w) == 1 and len(bodies(w[10], (2, 1))) == 1
    return r


HDR_PROPS = {"headers": {"kind": "late", "n": 7}, "content_type": "text/plain", "delivery_mode": 1}


def sc_record_bytes(dp, on=True):
    """Bodies of 0, 1, 15, 16, 17 bytes and one of several KB, a 255-byte key and a 255-byte exchange
    name, properties with a headers table: property bytes and body arrive verbatim, the Deliver
    names the dead-letter exchange, and the key is the message's own or x-dead-letter-routing-key."""
    r = Rec(dp, on, TTL_STEP)
    long_x, long_k = "X" * 255, "k" * 255
    r.exchange(long_x, "fanout")
    r.exchange("dx", "direct")
    r.queue("park")
    r.queue("park2")
    r.bind("park", long_x)
    r.bind("park2", "dx", long_k)
    r.queue("own", dlx=long_x)
    r.queue("keyed", dlx="dx", dlk=long_k)
    r.open(1)
    r.consume(2, 1, "park")
    r.consume(2, 2, "park2")
    for size in (0, 1, 15, 16, 17, 5000):
        body = bytes((i * 7 + size) & 255 for i in range(size))
        r.pub(1, 1, 1, "own", expire_ms=1000, body=body, props=HDR_PROPS)
        r.pub(1, 1, 1, "keyed", expire_ms=1000, body=body)
    r.end(4)
    w = r.want
    if on:
        assert [len(e[4]) for e in w[3]["events"][(2, 1)]] == [0, 1, 15, 16, 17, 5000]
        assert all(e[1] == long_x and e[2] == b"own" and e[3]["headers"] == HDR_PROPS["headers"]
                   and e[3]["expiration"] == "1000" for e in w[3]["events"][(2, 1)])
        assert all(e[1] == "dx" and e[2] == long_k.encode() for e in w[3]["events"][(2, 2)])
    return r


def sc_routing(dp, on=True):
    """A fanout dead-letter exchange to two queues; a topic one matched by x-dead-letter-routing-key;
    one reached over an exchange-to-exchange edge; one deleted after the declare (n_dl_unrouted) and
    one declared only later (the slot is looked up again); a route to no queue (n_dl_unrouted)."""
    r = Rec(dp, on, TTL_STEP)
    r.exchange("fan", "fanout")
    r.exchange("top", "topic")
    r.exchange("hub", "fanout")
    r.exchange("gone", "fanout")
    r.exchange("void", "direct")
    for q in ("f1", "f2", "t1", "h1", "late1", "g1"):
        r.queue(q)
    r.bind("f1", "fan")
    r.bind("f2", "fan")
    r.bind("t1", "top", "dead.*.eu")
    r.bind_x("fan", "hub")                 # hub -> fan -> f1, f2
    r.bind("h1", "hub")
    r.bind("g1", "gone")
    specs = dict(qf=("fan", None), qt=("top", "dead.orders.eu"), qm=("top", "dead.orders.us"), qh=("hub", None),
                 qg=("gone", None), ql=("late", None), qv=("void", None))
    for q, (x, k) in specs.items():
        r.queue(q, dlx=x, dlk=k)
    r.open(1)
    for c, q in enumerate(("f1", "f2", "t1", "h1", "late1", "g1")):
        r.consume(2, c + 1, q)
    for q in specs:
        r.pub(1, 1, 2, q, expire_ms=1000)
    r.delete_exchange("gone")
    r.end()
    r.exchange("late", "fanout", later=True)
    r.ops.append(("bind", (VH, "late1", "late", ""), {}))
    r.x["late"]["binds"].append(("late1", b"", None))
    r.end(3)
    w = r.want
    if on:
        c2 = w[2]["counters"]
        assert c2["n_dl_expired"] == 12 and c2["n_dl_unrouted"] == 2          # qg: no exchange when they died
        assert w[3]["counters"]["n_dl_unrouted"] == 4                       # qm, qv: routed to no queue
        assert len(bodies(w[3], (2, 1))) == 4 and len(bodies(w[3], (2, 2))) == 4 and len(bodies(w[3], (2, 4))) == 2
        assert bodies(w[3], (2, 3)) == [body_of("qt", i) for i in range(2)]
        assert bodies(w[3], (2, 5)) == [body_of("ql", i) for i in range(2)] and not bodies(w[3], (2, 6))
    return r


def sc_headers_dlx(dp, on=True):
    """A headers dead-letter exchange (headers_match on): the dead letter is matched on its own
    property bytes' headers table."""
    r = Rec(dp, on, TTL_STEP)
    r.exchange("hx", "headers")
    r.queue("late")
    r.queue("other")
    r.bind("late", "hx", "", args={"x-match": "all", "kind": "late"},
           pred=lambda rk, p: (p.get("headers") or {}).get("kind") == "late")
    r.bind("other", "hx", "", args={"x-match": "all", "kind": "other"},
           pred=lambda rk, p: (p.get("headers") or {}).get("kind") == "other")
    r.queue("src", dlx="hx")
    r.open(1)
    r.consume(2, 1, "late")
    r.consume(2, 2, "other")
    r.pub(1, 1, 3, "src", expire_ms=1000, props=HDR_PROPS)
    r.pub(1, 1, 1, "src", expire_ms=1000, props={"headers": {"kind": "none"}})
    r.end(4)
    if on:
        assert len(bodies(r.want[3], (2, 1))) == 3 and not bodies(r.want[3], (2, 2))
        assert r.want[3]["counters"]["n_dl_unrouted"] == 1
    return r


def sc_chain(dp, on=True):
    """TTL queue -> exchange -> a queue with L = 1 and its own dead-letter exchange -> third queue:
    one hop per step.  And a queue that dead-letters into itself: cycles are not detected (there is
    no x-death header yet, which is what detection needs: the follow-up), so its message goes
    round -- it dies in one step and is back in the queue in the next, three times here."""
    r = Rec(dp, on, TTL_STEP)
    r.exchange("x1", "fanout")
    r.exchange("x2", "fanout")
    r.exchange("loop", "fanout")
    r.queue("first", ttl=500, dlx="x1")
    r.queue("second", L=1, dlx="x2")
    r.queue("third")
    r.queue("self", ttl=500, dlx="loop")
    r.bind("second", "x1")
    r.bind("third", "x2")
    r.bind("self", "loop")
    r.open(1)
    r.pub(1, 1, 3, "first")
    r.pub(1, 1, 1, "self")
    r.end(7)
    r.consume(2, 1, "third", later=True)
    r.consume(2, 2, "second", later=True)
    r.end(2)
    w = r.want
    if on:
        s = {n: r.q[n]["slot"] for n in r.q}
        assert [x["depth"][s["second"]] for x in w[:4]] == [0, 0, 1, 1]
        assert [x["depth"][s["third"]] for x in w[:5]] == [0, 0, 0, 2, 2]
        assert [x["counters"]["n_dl_expired"] for x in w[:7]] == [0, 4, 0, 1, 0, 1, 0]    # the loop: three times round
        assert all(x["depth"][s["self"]] + x["counters"]["n_dl_pending"] >= 1 for x in w)   # and never lost
        assert w[2]["counters"]["n_dl_maxlen"] == 2
        assert bodies(w[7], (2, 1)) == [body_of("first", i) for i in (0, 1)] and bodies(w[7], (2, 2)) == [body_of("first", 2)]
    return r


def sc_non_exits(dp, on=True):
    """Purge of a queue with a dead-letter exchange, delete of one, a reject-publish refusal: none of
    them dead-letters anything."""
    r = Rec(dp, on)
    r.exchange("dlx", "fanout")
    r.queue("park")
    r.bind("park", "dlx")
    r.queue("purged", dlx="dlx")
    r.queue("deleted", dlx="dlx")
    r.queue("full", L=2, mode="reject-publish", dlx="dlx")
    r.open(1)
    r.pub(1, 1, 70, "purged")
    r.pub(1, 1, 5, "deleted")
    r.pub(1, 1, 6, "full")
    r.end()
    r.purge("purged")
    r.purge("deleted")
    r.end()
    r.delete_queue("deleted")
    r.end(2)
    w = r.want
    assert w[0]["counters"]["n_maxlen_rejected"] == 4 and w[1]["counters"]["n_expired"] == 75
    assert all(x["depth"][r.q["park"]["slot"]] == 0 for x in w)
    assert all(x["counters"][c] == 0 for x in w for c in COUNTERS if c.startswith("n_dl_"))
    return r


PERSIST_CFG = dict(persist=1, persist_max=4096, persist_bytes=8 << 20, deliv_max=512, pair_max=8192, queue_limits=True,
                   restore_max=64)


def sc_durable(dp, on=True):
    """A persisting plane, durable source and target, persistent messages: the source's consumed
    record (kind 1 for an expired entry, 0 for a rejected one) is written when the entry dies,
    the target's persist record when the dead letter is enqueued a step later."""
    r = Rec(dp, on, TTL_STEP, persist_budget=1280)
    r.exchange("dlx", "fanout")
    r.queue("park", durable=True)
    r.bind("park", "dlx")
    r.queue("src", durable=True, dlx="dlx")
    r.queue("work", durable=True, dlx="dlx")
    r.open(1)
    r.consume(3, 1, "work", no_ack=False)
    r.pub(1, 1, 3, "src", expire_ms=1000, props=PERSISTENT)
    r.pub(1, 1, 1, "src", expire_ms=1000)                     # transient: no records
    r.pub(1, 1, 2, "work", props=PERSISTENT)
    r.end()
    r.settle(3, 1, "reject", 2)
    r.end(2)
    r.consume(2, 1, "park", later=True)
    r.end()
    r.settle(3, 1, "ack", 1)
    r.end()
    w = r.want
    if on:
        s = {n: r.q[n]["slot"] for n in r.q}
        assert w[1]["consumed"] == [(s["work"], 1, 0)] and w[2]["consumed"] == [(s["src"], i, 1) for i in range(3)]
        assert [x[:2] for x in w[2]["stored"]] == [(s["park"], 0)] and [x[:2] for x in w[3]["stored"]] == [(s["park"], i) for i in (1, 2, 3)]
        assert all(x[2] == b"dlx" for x in w[3]["stored"])
    return r


BUDGET_CFG = dict(PERSIST_CFG, dead_max=LIST_MAX, cmd_max=4096)


def sc_list_and_budget(dp, on=True):
    """The list full together with the TTL walk's record budget (1280 a step, reserved 64 at a time):
    a durable queue without a dead-letter exchange takes 19 reservations for its 1216 expired
    entries, the durable queue behind it one for 64 of its 100 -- which fill the list of 64 -- and
    finds no budget for the rest: they stay queued and go in the next steps."""
    r = Rec(dp, on, TTL_STEP, dead_max=LIST_MAX, persist_budget=1280)
    r.exchange("dlx", "fanout")
    r.queue("park")
    r.bind("park", "dlx")
    r.queue("bulk", durable=True, capacity=2048)
    r.queue("src", durable=True, dlx="dlx")
    r.open(1)
    r.pub(1, 1, 1216, "bulk", expire_ms=1000, props=PERSISTENT)
    r.pub(1, 1, 100, "src", expire_ms=1000, props=PERSISTENT)
    r.end(3)
    r.consume(2, 1, "park", later=True)
    r.end(3)
    w = r.want
    if on:
        assert w[2]["counters"]["n_expired"] == 1216 + 64 and w[2]["counters"]["n_dl_expired"] == 64
        assert w[2]["depth"][r.q["src"]["slot"]] == 36 and w[3]["counters"]["n_dl_expired"] == 36
        assert sum((bodies(x, (2, 1)) for x in w), []) == [body_of("src", i) for i in range(100)]
    return r


def sc_off(dp, on=False):
    """The same declares with the option off: the arguments are ignored, expired and trimmed
    entries are released, a reject without requeue is an ack, no counter of the feature moves."""
    r = Rec(dp, False, TTL_STEP)
    r.exchange("dlx", "fanout")
    r.queue("park")
    r.bind("park", "dlx")
    r.queue("t", dlx="dlx", dlk="k")
    r.queue("w", dlx="dlx")
    r.open(1)
    r.consume(3, 1, "w", no_ack=False)
    r.consume(2, 1, "park")
    r.pub(1, 1, 5, "t", expire_ms=1000)
    r.pub(1, 1, 2, "w")
    r.end()
    r.settle(3, 1, "reject", 1)
    r.settle(3, 1, "nack", 2, multiple=True)
    r.end(3)
    assert all(x["counters"][c] == 0 for x in r.want for c in COUNTERS if c.startswith("n_dl_"))
    assert r.want[2]["counters"]["n_expired"] == 5 and not any(x["events"] for x in r.want[1:])
    return r


TWO_PASS = dict(q_max=4096)    # a pair key above SORT_ONEPASS_BITS: k_ring_plan + k_enqueue instead of the fused sort
SMALL_LIST = dict(dead_max=LIST_MAX)
SCENARIOS = {
    "ttl_edges": Scenario(sc_ttl_edges, {}, TTL_STEP, False),
    "trim": Scenario(sc_trim, dict(queue_limits=True), 0, False),
    "rejects": Scenario(sc_rejects, {}, 0, True),
    "reject_fold": Scenario(sc_reject_fold, dict(ucap=512), 0, True),
    "list_63": Scenario(lambda dp, on=True: sc_list_limits(dp, on, -1), dict(SMALL_LIST, dead_bytes=10 * REC), TTL_STEP, True),
    "list_64": Scenario(lambda dp, on=True: sc_list_limits(dp, on, 0), dict(SMALL_LIST, dead_bytes=10 * REC), TTL_STEP, True),
    "list_65": Scenario(lambda dp, on=True: sc_list_limits(dp, on, 1), dict(SMALL_LIST, dead_bytes=10 * REC), TTL_STEP, True),
    "reject_deferred": Scenario(sc_reject_deferred, dict(dead_max=16, dead_bytes=2 * REC), TTL_STEP, True),
    "payload": Scenario(sc_payload, dict(dead_bytes=4 * REC), TTL_STEP, True),
    "record_bytes": Scenario(sc_record_bytes, {}, TTL_STEP, True),
    "routing": Scenario(sc_routing, {}, TTL_STEP, True),
    "both_paths_routing": Scenario(sc_routing, TWO_PASS, TTL_STEP, True),
    "headers_dlx": Scenario(sc_headers_dlx, dict(headers_match=True), TTL_STEP, True),
    "chain": Scenario(sc_chain, dict(queue_limits=True), TTL_STEP, False),
    "non_exits": Scenario(sc_non_exits, dict(queue_limits=True), 0, False),
    "durable": Scenario(sc_durable, PERSIST_CFG, TTL_STEP, True),
    "list_and_budget": Scenario(sc_list_and_budget, BUDGET_CFG, TTL_STEP, True),
}
OFF = Scenario(sc_off, {}, TTL_STEP, True)
