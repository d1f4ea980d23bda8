"""x-death headers and cycle detection (``x_death=True`` on top of ``dead_letter=True``) in the
``dlx_scenarios`` style: each scenario is ``dp -> XRec`` with its own engine overrides.

``XRec`` is ``dlx_scenarios.Rec`` with a dead pass of its own.  It predicts every delivery's
**property bytes**: the expected headers are built as Python dicts with ``Typed('l', ..)`` /
``Typed('T', ..)`` values (``predict`` below, the rule as CHANGES.md "x-death headers" states it)
and encoded with protocol/codec.py, which keeps insertion order.  It never calls the golden model's
rewrite (chanamq_amd/engine/xdeath.py works on bytes; this works on dicts).  ``check`` judges the
golden model's run and the HIP data plane's alike.
"""

from collections import defaultdict

from chanamq_amd.protocol.codec import FrameParser, Typed, decode_content_header, decode_method, encode_properties
from dlx_scenarios import (COUNTERS as DLX_COUNTERS, DELIVER_CAP, EXPIRED, MAXLEN, PERSIST_CFG, REJECTED, TTL_STEP, Entry,
                           Rec, Scenario, a16, bodies, persists)
from consumer_scenarios import GOLDEN_KEYS, body_of
from dp_scenarios import NOW, VH

COUNTERS = DLX_COUNTERS + ("n_dl_cycle",)
REASON = ("expired", "maxlen", "rejected")
ELEMS_MAX, PROPS_MAX = 64, 65535
INT_TAGS = "bBsuIil"


def _b(k):
    return k if isinstance(k, bytes) else k.encode()


def _s(e, k):
    v = e.get(k)
    return v if isinstance(v, str) else None


def predict(props, qname, reason, ex, rk, time_s):
    """The dead letter's properties (a dict; None: over a limit, dropped) and the queue names its
    history bans, from the message's properties and what died."""
    p = dict(props)
    exp = p.pop("expiration", None)
    old = p.get("headers") or {}
    h = {k: v for k, v in old.items() if _b(k) != b"x-death"}
    xds = [v for k, v in old.items() if _b(k) == b"x-death"]
    arr = xds[0] if xds else []
    if not isinstance(arr, list) or not all(isinstance(e, dict) for e in arr):
        arr = []
    rs = REASON[reason]
    m = next((i for i, e in enumerate(arr) if _s(e, "queue") == qname and _s(e, "reason") == rs), None)
    if m is None:
        front = {"count": Typed("l", 1), "reason": rs, "queue": qname, "time": Typed("T", time_s), "exchange": ex,
                 "routing-keys": [rk]}
        if exp is not None:
            front["original-expiration"] = exp
        rest = list(arr)
    else:
        c = arr[m].get("count")
        if isinstance(c, Typed) and c.tag in INT_TAGS:
            n = c.value + 1
        elif isinstance(c, int) and not isinstance(c, bool):
            n = c + 1
        else:
            n = 1
        front = dict(arr[m]) if "count" in arr[m] else {"count": None, **arr[m]}
        front["count"] = Typed("l", n)
        rest = arr[:m] + arr[m + 1:]
    merged = [front] + rest
    if len(merged) > ELEMS_MAX:
        return None, []
    if not any(_b(k) == b"x-first-death-queue" for k in h):
        h.update({"x-first-death-reason": rs, "x-first-death-queue": qname, "x-first-death-exchange": ex})
    h["x-death"] = merged
    p["headers"] = h
    if len(encode_properties(p)) > PROPS_MAX:
        return None, []
    bans = []
    for e in merged:
        if _s(e, "queue") is None or _s(e, "reason") is None:
            continue
        if e["reason"] == "rejected":
            break
        bans.append(e["queue"])
    return p, bans


def raw_props(props):
    return encode_properties(props or {})


class XRec(Rec):
    """``Rec`` whose dead pass rewrites the properties and refuses banned queues.  Events carry the
    property *bytes*; ``self.died`` lists every rendered dead letter's new properties."""

    def __init__(self, dp, *a, **kw):
        super().__init__(dp, True, *a, **kw)
        self.died = []

    def _join(self, qn, e, qpos, reason, k, ch, tag, cnt):
        super()._join(qn, e, qpos, reason, k, ch, tag, cnt)
        self.dead[-1]["qn"] = qn

    def _end(self):
        # dlx_scenarios.Rec._end (which may not be edited) with these differences: (2) the dead pass
        # predicts each item's new properties, sizes the prefix by them and refuses banned queues;
        # (3) single settles only; (4) no persist-record budget; events carry property bytes, not dicts
        k = len(self.steps)
        now = NOW + self.now_step_ms * k
        cnt = dict.fromkeys(COUNTERS, 0)
        ev = defaultdict(list)
        self.stored, self.consumed = [], []
        # (1) the step's own publishes, in publish order (connection, then wire order)
        for conn, _, ex, rk, body, props, exp_ms in sorted(self.pubs, key=lambda p: p[:2]):
            e = Entry(ex, rk, props, body, now + exp_ms if exp_ms else 0, 0, len(raw_props(props)))
            for qn in sorted(self.route(ex, rk, props), key=lambda n: self.q[n]["slot"]):
                self._enqueue(qn, e, now, cnt)
        # (2) the dead pass: each pending item's new properties first -- the prefix is that of the
        # new sizes -- then the items in their order as far as the pass's room goes
        self.dead.sort(key=lambda d: (d["step"], d["q"], d["qpos"], d["reason"], d["ch"], d["tag"]))
        take = nrec = nbytes = 0
        for d in self.dead:
            e = d["e"]
            d["np"], d["bans"] = predict(e.props, d["qn"], d["reason"], e.ex, e.rk, now // 1000)
            if d["np"] is None:
                d["size"] = self.dead_bytes + 1
            else:
                d["size"] = a16(a16(len(d["ex"].encode()) + len(d["rk"]) + len(raw_props(d["np"]))) + len(e.body))
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
            self.died.append(d["np"])
            qs = self.route(d["ex"], d["rk"], d["np"]) if d["ex"] in self.x else set()
            refused = {q for q in qs if q in d["bans"]}
            cnt["n_dl_cycle"] += len(refused)
            qs -= refused
            if not qs:
                cnt["n_dl_unrouted"] += 1
            e = Entry(d["ex"], d["rk"], d["np"], d["e"].body, 0, 0, len(raw_props(d["np"])))
            for qn in sorted(qs, key=lambda n: self.q[n]["slot"]):
                self._enqueue(qn, e, now, cnt)
        # (3) settles (the scenarios here use single rejects, acks and requeues only)
        back = defaultdict(list)
        for key in sorted(self.chan):
            c = self.chan[key]
            for _, _, kind, tag, multiple in (s for s in self.settles if s[:2] == key):
                assert not multiple
                for u in c["unacked"]:
                    if u["tag"] == tag and u["mark"] is None:
                        u["mark"] = kind
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
                    if q["dlx"] in self.x:
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
        for qn, q in sorted(self.q.items(), key=lambda kv: kv[1]["slot"]):
            items = q["items"]
            while items and items[0].expire and items[0].expire <= now:
                assert self._leave(qn, items[0], q["head"], EXPIRED, k, cnt)
                items.pop(0)
                q["head"] += 1
                cnt["n_expired"] += 1
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
                    ev[(c["conn"], c["ch"])].append((c["tag"], e.ex, e.rk, raw_props(e.props), e.body, e.red, chan["tag"]))
                    cnt["n_deliv"] += 1
                del items[:g]
                q["head"] += g
            if q["L"] is not None and q["mode"] == "drop-head":
                while len(items) > q["L"]:
                    assert self._leave(qn, items[0], q["head"], MAXLEN, k, cnt)
                    items.pop(0)
                    q["head"] += 1
                    cnt["n_maxlen_dropped"] += 1
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

    def _enqueue(self, qn, e, now, cnt):
        n0 = len(self.stored) if hasattr(self, "stored") else 0
        super()._enqueue(qn, e, now, cnt)
        if hasattr(self, "stored") and len(self.stored) > n0:   # the store record with its property bytes
            self.stored[-1] = self.stored[-1][:4] + (raw_props(e.props),) + self.stored[-1][4:]


# ---------------------------------------------------------------- planes and runner
DL_KEYS = ("dead_max", "dead_bytes", "restore_max")


def golden_plane(cfg):
    from chanamq_amd.engine.golden import GoldenDataPlane
    kw = {k: cfg[k] for k in GOLDEN_KEYS + ("ring_pool", "deliv_max", "egress_cap", "persist_max") if k in cfg}
    if cfg.get("persist"):
        kw["persist"] = True
    for k in ("queue_limits", "headers_match"):
        if cfg.get(k):
            kw[k] = True
    kw.update(dead_letter=True, x_death=True, **{k: cfg[k] for k in DL_KEYS if k in cfg})
    return GoldenDataPlane(**kw)


def gpu_plane(cfg, graph):
    from chanamq_amd.engine.dataplane import GpuDataPlane
    return GpuDataPlane(graph=graph, **dict(cfg, dead_letter=True, x_death=True))


def run_xd(dp, rec):
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
        if persists(dp):
            o["stored"] = sorted((int(p[2]), int(p[3]), bytes(p[5]), bytes(p[6]), bytes(p[7]), bytes(p[8])) for p in dp.take_persist())
            o["consumed"] = sorted((int(q), int(qpos), int(kind)) for _, q, qpos, kind in dp.take_consumed())
        outs.append(o)
    return outs


def observe(out, k):
    """One step's deliveries: {(conn, ch): [(consumer tag, exchange, routing key, property bytes,
    body, redelivered, delivery tag)]}; anything else on the wire fails."""
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
                _, cur[2], _ = decode_content_header(fr.payload)
                cur[4] = bytes(fr.payload[12:])
            else:
                cur[3].append(fr.payload)
            if cur[2] is not None and sum(map(len, cur[3])) >= cur[2]:
                m = cur[1]
                rk = m.routing_key if isinstance(m.routing_key, bytes) else m.routing_key.encode()
                ev[(conn, cur[0])].append((m.consumer_tag, m.exchange, rk, cur[4], b"".join(cur[3]), bool(m.redelivered),
                                           m.delivery_tag))
                cur = None
        assert cur is None and not fp.buf, f"step {k} conn {conn}: egress ends inside a command"
    return dict(ev)


def _show(raw):
    from chanamq_amd.protocol.codec import decode_properties
    try:
        return decode_properties(raw)[0]
    except Exception as e:   # noqa: BLE001
        return f"{raw[:64].hex()}.. ({e})"


def check(rec, outs):
    """The run against the record, step by step."""
    assert len(outs) == len(rec.want)
    for k, (o, w) in enumerate(zip(outs, rec.want)):
        ev = observe(o, k)
        assert sorted(ev) == sorted(w["events"]), f"step {k}: deliveries on {sorted(ev)}, expected on {sorted(w['events'])}"
        for key in ev:
            g, x = ev[key], w["events"][key]
            assert [e[4] for e in g] == [e[4] for e in x], f"step {k} {key}: bodies differ"
            for a, b in zip(g, x):
                assert a[3] == b[3], f"step {k} {key}: property bytes of {a[4][:24]}: got {_show(a[3])}, expected {_show(b[3])}"
            assert g == x, f"step {k} {key}: deliveries differ"
        assert o["counters"] == w["counters"], f"step {k}: counters {o['counters']}, expected {w['counters']}"
        assert o["depth"] == w["depth"], f"step {k}: depths {o['depth']}, expected {w['depth']}"
        if "consumed" in w:
            assert o["consumed"] == w["consumed"], f"step {k}: consumed records {o['consumed']}, expected {w['consumed']}"
            assert o["stored"] == w["stored"], f"step {k}: persist records differ"


def xdeath_of(raw):
    """The decoded x-death array of a delivery's property bytes."""
    from chanamq_amd.protocol.codec import decode_properties
    return decode_properties(raw)[0]["headers"]["x-death"]


# ---------------------------------------------------------------- scenarios
BOTH_SIDES = {"content_type": "text/plain", "delivery_mode": 1, "correlation_id": "c-1", "timestamp": 1_700_000_123}


def park(r, dlx="dlx", type_="fanout", consume=True):
    r.exchange(dlx, type_)
    r.queue("park")
    r.bind("park", dlx)
    r.open(1)
    if consume:
        r.consume(2, 1, "park")


def sc_first_death(dp):
    """One message per reason, each without a headers property, with one, and with properties on both
    sides of it: the table is created or extended, flag bit 13 set and bit 8 cleared, the expiration
    removed for every reason and remembered as original-expiration."""
    r = XRec(dp, TTL_STEP)
    park(r)
    r.queue("ttl", dlx="dlx")
    r.queue("trim", L=0, dlx="dlx")
    r.queue("work", dlx="dlx")
    r.consume(3, 1, "work", no_ack=False)
    variants = ({}, {"headers": {"kind": "late", "n": 7}}, dict(BOTH_SIDES, headers={"a": "b"}), dict(BOTH_SIDES))
    for v in variants:
        r.pub(1, 1, 1, "ttl", props=v, expire_ms=1000)
        r.pub(1, 1, 1, "trim", props=v, expire_ms=60000)
        r.pub(1, 1, 1, "work", props=v, expire_ms=60000)
    r.end()
    for t in range(1, len(variants) + 1):
        r.settle(3, 1, "reject", t)
    r.end(4)
    assert len(r.died) == 12
    for p in r.died:
        assert "expiration" not in p and list(p["headers"])[-4:] == ["x-first-death-reason", "x-first-death-queue",
                                                                     "x-first-death-exchange", "x-death"]
        x = p["headers"]["x-death"]
        assert len(x) == 1 and x[0]["count"] == Typed("l", 1) and x[0]["original-expiration"] in ("1000", "60000")
        assert list(x[0]) == ["count", "reason", "queue", "time", "exchange", "routing-keys", "original-expiration"]
    assert sorted(p["headers"]["x-death"][0]["reason"] for p in r.died) == sorted(REASON * 4)
    assert sum(len(bodies(w, (2, 1))) for w in r.want) == 12
    return r


def sc_recount(dp):
    """A consumer rejects through work -> dlx -> work four times: one element whose count goes 1, 2,
    3, 4 while its time stays that of the first death (the steps are 600 ms apart).  An expiry in this
    same queue would be refused on its way back -- work's own entry, no reject in front of it, bans
    work -- so the second element and the move back to the front are `recount_mixed`'s, over two queues."""
    r = XRec(dp, TTL_STEP)
    r.exchange("dlx", "fanout")
    r.queue("work", dlx="dlx")
    r.bind("work", "dlx")
    r.open(1)
    r.consume(3, 1, "work", no_ack=False)
    r.pub(1, 1, 1, "work", props={"headers": {"job": 4}})
    r.end()
    for t in (1, 2, 3, 4):
        r.settle(3, 1, "reject", t)
        r.end(2)
    assert [p["headers"]["x-death"][0]["count"].value for p in r.died] == [1, 2, 3, 4]
    assert len({p["headers"]["x-death"][0]["time"].value for p in r.died}) == 1
    assert all(len(p["headers"]["x-death"]) == 1 for p in r.died)
    return r


def sc_recount_mixed(dp):
    """Reject in `a` (-> b), expiry in `b` (-> a), reject in `a` again: the second death puts a new
    element in front, the third moves a's element back to the front with count 2, b's follows."""
    r = XRec(dp, TTL_STEP)
    r.exchange("xa", "fanout")
    r.exchange("xb", "fanout")
    r.queue("a", dlx="xb")
    r.queue("b", dlx="xa", ttl=500)
    r.bind("a", "xa")
    r.bind("b", "xb")
    r.open(1)
    r.consume(3, 1, "a", no_ack=False)
    r.pub(1, 1, 1, "a")
    r.end()
    r.settle(3, 1, "reject", 1)
    r.end(5)                      # -> b, expires there, back in a (the reject in front lifts the ban), delivered
    r.settle(3, 1, "reject", 2)
    r.end(2)
    seq = [[(e["queue"], e["reason"], e["count"].value) for e in p["headers"]["x-death"]] for p in r.died]
    assert seq[:3] == [[("a", "rejected", 1)], [("b", "expired", 1), ("a", "rejected", 1)],
                       [("a", "rejected", 2), ("b", "expired", 1)]], seq
    return r


LOOKALIKES = {"x-deat": "1", "x-death2": [{"queue": "q", "reason": "expired"}], "X-Death": 5}


def sc_names(dp):
    """Queue names of 1 and 255 bytes, routing keys of 0 and 255 bytes, a publish to the default
    exchange (an empty exchange field), header names that only look like x-death, and a duplicate
    x-death entry (the first is read, both are removed)."""
    r = XRec(dp, TTL_STEP)
    park(r)
    long_q, long_k = "Q" * 255, "k" * 255
    r.exchange("in", "fanout")
    r.queue("q", dlx="dlx")
    r.queue(long_q, dlx="dlx")
    r.bind("q", "in")
    r.bind(long_q, "in")
    r.pub(1, 1, 1, exchange="in", key="", expire_ms=1000, props={"headers": dict(LOOKALIKES)})
    r.pub(1, 1, 1, exchange="in", key=long_k, expire_ms=1000)
    r.pub(1, 1, 1, "q", expire_ms=1000)
    first = [{"count": Typed("l", 5), "reason": "expired", "queue": "q"}]
    r.pub(1, 1, 1, "q", expire_ms=1000, props={"headers": {"x-death": first, "mid": 1, b"x-death": "second"}})
    r.end(4)
    assert len(r.died) == 6
    dup = [p for p in r.died if "mid" in p["headers"]][0]
    assert list(dup["headers"])[0] == "mid" and dup["headers"]["x-death"][0]["count"] == Typed("l", 6)
    assert all(k in p["headers"] for p in r.died if "x-deat" in p["headers"] for k in LOOKALIKES)
    assert {p["headers"]["x-death"][0].get("exchange") for p in r.died} == {"in", "", None}
    return r


def element(i, reason="expired"):
    return {"count": Typed("l", 1), "reason": reason, "queue": f"old{i}", "time": Typed("T", 1_600_000_000 + i),
            "exchange": "", "routing-keys": [f"old{i}"]}


def sc_client_arrays(dp):
    """Publishes that arrive with an x-death of 62, 63 and 64 elements: merged to 63 and 64, the last
    dropped (n_dl_dropped); 64 elements of which one matches the new death stay 64 and are kept.
    Malformed values (a string, an array holding an integer, a table without `queue`), and an
    existing x-first-death-queue, which is left alone."""
    r = XRec(dp, TTL_STEP)
    park(r)
    r.queue("q", dlx="dlx")
    for n in (62, 63, 64):
        r.pub(1, 1, 1, "q", expire_ms=1000, props={"headers": {"x-death": [element(i) for i in range(n)]}})
    own = {"count": 7, "reason": "expired", "queue": "q"}
    r.pub(1, 1, 1, "q", expire_ms=1000, props={"headers": {"x-death": [element(i) for i in range(63)] + [own]}})
    r.pub(1, 1, 1, "q", expire_ms=1000, props={"headers": {"x-death": "once"}})
    r.pub(1, 1, 1, "q", expire_ms=1000, props={"headers": {"x-death": [element(0), 5]}})
    r.pub(1, 1, 1, "q", expire_ms=1000, props={"headers": {"x-death": [{"reason": "expired", "n": 1}, element(1)]}})
    r.pub(1, 1, 1, "q", expire_ms=1000, props={"headers": {"x-first-death-queue": "elsewhere", "x-death": [element(2)]}})
    r.end(4)
    assert sum(w["counters"]["n_dl_dropped"] for w in r.want) == 1
    lens = [len(p["headers"]["x-death"]) for p in r.died]
    assert lens == [63, 64, 64, 1, 1, 3, 2], lens
    assert r.died[2]["headers"]["x-death"][0] == {"count": Typed("l", 8), "reason": "expired", "queue": "q"}
    assert r.died[5]["headers"]["x-death"][1] == {"reason": "expired", "n": 1}
    assert r.died[6]["headers"]["x-first-death-queue"] == "elsewhere" and "x-first-death-reason" not in r.died[6]["headers"]
    return r


def _pad_to(total, qname="q", rk=b"q"):
    """A headers value that makes the dead letter's property bytes exactly ``total``."""
    base = predict({"headers": {"pad": ""}, "expiration": "1000"}, qname, EXPIRED, "", rk, 0)[0]
    return "p" * (total - len(raw_props(base)))


def sc_size_bound(dp):
    """Rewritten property bytes of exactly the bound (65535) fit; one more byte is dropped."""
    r = XRec(dp, TTL_STEP)
    park(r)
    r.queue("q", dlx="dlx")
    r.pub(1, 1, 1, "q", expire_ms=1000, props={"headers": {"pad": _pad_to(PROPS_MAX)}})
    r.pub(1, 1, 1, "q", expire_ms=1000, props={"headers": {"pad": _pad_to(PROPS_MAX + 1)}})
    r.end(4)
    assert len(r.died) == 1 and len(raw_props(r.died[0])) == PROPS_MAX
    assert sum(w["counters"]["n_dl_dropped"] for w in r.want) == 1
    return r


PREFIX_N = 4


def prefix_bytes():
    """A dead_bytes that holds PREFIX_N records of sc_prefix by their new size and PREFIX_N + 1 by
    their old one."""
    old = a16(a16(3 + 1 + len(raw_props({"expiration": "1000"}))) + 30)
    new = a16(a16(3 + 1 + len(raw_props(predict({"expiration": "1000"}, "q", EXPIRED, "", b"q", 0)[0]))) + 30)
    assert PREFIX_N * new >= (PREFIX_N + 1) * old
    return PREFIX_N * new


def sc_prefix(dp):
    """PREFIX_N + 1 entries die in one step: by their old size they would all fit dead_bytes, by the
    new one only PREFIX_N -- the last goes a step later: the prefix uses the new size."""
    r = XRec(dp, TTL_STEP, dead_bytes=prefix_bytes())
    park(r)
    r.queue("q", dlx="dlx")
    r.pub(1, 1, PREFIX_N + 1, "q", expire_ms=1000, size=30)
    r.end(5)
    assert [len(bodies(w, (2, 1))) for w in r.want[3:5]] == [PREFIX_N, 1]
    return r


def sc_cycles(dp):
    """A queue that dead-letters into itself by TTL: the dead letter is refused at once (n_dl_cycle
    1) and the queue stays empty.  The same loop by reject keeps going.  a -> b -> a by TTL is
    refused on the return; with a reject in b it passes."""
    r = XRec(dp, TTL_STEP, room=64)
    for x in ("loop", "rloop", "xa", "xb", "ya", "yb"):
        r.exchange(x, "fanout")
    r.queue("self", ttl=500, dlx="loop")
    r.bind("self", "loop")
    r.queue("rself", dlx="rloop")
    r.bind("rself", "rloop")
    r.queue("a", ttl=500, dlx="xb")
    r.queue("b", ttl=500, dlx="xa")
    r.bind("a", "xa")
    r.bind("b", "xb")
    r.queue("c", ttl=500, dlx="yb")
    r.queue("d", dlx="ya")
    r.bind("c", "ya")
    r.bind("d", "yb")
    r.open(1)
    r.consume(3, 1, "rself", no_ack=False)
    r.consume(4, 1, "d", no_ack=False)
    for q in ("self", "rself", "a", "c"):
        r.pub(1, 1, 1, q)
    r.end(2)
    r.settle(3, 1, "reject", 1)
    r.end(2)
    r.settle(4, 1, "reject", 1)
    r.settle(3, 1, "reject", 2)
    r.end(5)
    w, s = r.want, {n: r.q[n]["slot"] for n in r.q}
    assert w[2]["counters"]["n_dl_cycle"] == 1 and all(x["depth"][s["self"]] == 0 for x in w[1:])
    assert w[4]["counters"]["n_dl_cycle"] == 1 and sum(x["counters"]["n_dl_cycle"] for x in w) == 2   # self; a -> b -> a
    assert len(sum((bodies(x, (4, 1)) for x in w), [])) == 2           # c -> d, rejected there, -> c -> d again
    assert len(sum((bodies(x, (3, 1)) for x in w), [])) >= 3           # the reject loop keeps going
    return r


def _target(r, i):
    """Queue t<i> with a consumer of its own (eight channels a connection)."""
    r.queue(f"t{i}")
    r.consume(2 + i // 8, i % 8 + 1, f"t{i}")


def got(w, i):
    return bodies(w, (2 + i // 8, i % 8 + 1))


def _ban_setup(r, type_, n):
    r.exchange("dlx", type_)
    r.open(1)
    for i in range(n):
        _target(r, i)


def sc_ban_direct(dp):
    """A banned queue among a direct exchange's two."""
    r = XRec(dp, TTL_STEP)
    _ban_setup(r, "direct", 1)
    r.bind("t0", "dlx", "k")
    r.queue("src", ttl=500, dlx="dlx", dlk="k")
    r.bind("src", "dlx", "k")
    r.pub(1, 1, 2, "src")
    r.end(4)
    assert r.want[2]["counters"]["n_dl_cycle"] == 2 and len(got(r.want[2], 0)) == 2
    return r


def sc_ban_fanout(dp):
    """A banned queue among a fanout's nine (more than PUB_QC: pass 1 routes again)."""
    r = XRec(dp, TTL_STEP)
    _ban_setup(r, "fanout", 4)
    for i in range(4):
        r.bind(f"t{i}", "dlx")
    r.queue("src", ttl=500, dlx="dlx")
    r.bind("src", "dlx")
    for i in range(4, 8):
        _target(r, i)
        r.bind(f"t{i}", "dlx")
    r.pub(1, 1, 2, "src")
    r.end(4)
    assert r.want[2]["counters"]["n_dl_cycle"] == 2 and r.want[2]["counters"]["n_deliv"] == 16
    return r


def sc_ban_topic(dp):
    """A banned queue among a topic exchange's."""
    r = XRec(dp, TTL_STEP)
    _ban_setup(r, "topic", 2)
    r.bind("t0", "dlx", "dead.#")
    r.queue("src", ttl=500, dlx="dlx", dlk="dead.src.eu")
    r.bind("src", "dlx", "dead.*.eu")
    r.bind("src", "dlx", "#")
    r.bind("t1", "dlx", "*.src.*")
    r.pub(1, 1, 2, "src")
    r.end(4)
    assert r.want[2]["counters"]["n_dl_cycle"] == 2 and r.want[2]["counters"]["n_deliv"] == 4
    return r


def sc_ban_hop(dp):
    """A banned queue behind an exchange-to-exchange edge with more than eight queues (hop_q)."""
    r = XRec(dp, TTL_STEP)
    _ban_setup(r, "fanout", 5)
    r.exchange("far", "fanout")
    r.bind_x("far", "dlx")
    for i in range(5):
        r.bind(f"t{i}", "far")
    r.queue("src", ttl=500, dlx="dlx")
    r.bind("src", "far")
    for i in range(5, 10):
        _target(r, i)
        r.bind(f"t{i}", "far" if i % 2 else "dlx")
    r.pub(1, 1, 2, "src")
    r.end(4)
    assert r.want[2]["counters"]["n_dl_cycle"] == 2 and r.want[2]["counters"]["n_deliv"] == 20
    return r


def sc_ban_headers(dp):
    """A headers dead-letter exchange (headers_match on) routes by the rewritten bytes, a banned queue
    among its rows: a message with properties on both sides of its table and one whose table the
    rewrite creates (it matches the row without pairs only).  A binding argument named
    x-first-death-reason is no pair -- arguments named x-* never are (CHANGES.md "Headers
    exchanges") -- so it matches whatever the reason.  That rule also means no binding can tell the
    rewritten bytes from the old ones: the rewrite changes x-* entries only, and a row without pairs
    matches with or without a table.  What this case holds is that the matcher walks the new bytes
    without fault and to the same queues -- the dead pass's record carries the new bytes alone, the
    old ones are not in it to be read."""
    r = XRec(dp, TTL_STEP)
    _ban_setup(r, "headers", 3)
    late = lambda rk, p: (p.get("headers") or {}).get("kind") == "late"   # noqa: E731
    r.bind("t0", "dlx", "", args={"x-match": "all", "kind": "late", "x-first-death-reason": "rejected"}, pred=late)
    r.bind("t1", "dlx", "", args={"x-match": "all", "kind": "other"},
           pred=lambda rk, p: (p.get("headers") or {}).get("kind") == "other")
    r.bind("t2", "dlx", "", args={"x-match": "all", "x-first-death-reason": "expired"}, pred=lambda rk, p: True)
    r.queue("src", ttl=500, dlx="dlx")
    r.bind("src", "dlx", "", args={"x-match": "all", "kind": "late"}, pred=late)
    r.pub(1, 1, 2, "src", props=dict(BOTH_SIDES, headers={"kind": "late"}, expiration="90000"))
    r.pub(1, 1, 1, "src")
    r.end(4)
    w = r.want[2]
    assert w["counters"]["n_dl_cycle"] == 2 and len(got(w, 0)) == 2 and not got(w, 1) and len(got(w, 2)) == 3
    return r


def sc_ban_many(dp):
    """40 banned dead letters rendered in one step that carries publishes of its own: the pass's
    records lie behind the step's publishes, more than one block of the pass's routing routes them
    (16 a block), and each finds its own ban row."""
    r = XRec(dp, TTL_STEP)
    _ban_setup(r, "fanout", 1)
    r.bind("t0", "dlx")
    r.queue("src", ttl=500, dlx="dlx")
    r.bind("src", "dlx")
    r.queue("other", dlx="dlx")
    r.pub(1, 1, 40, "src")
    r.pub(1, 1, 3, "other", expire_ms=500)       # not banned anywhere but in `other`: they reach src and t0
    r.end(2)
    r.pub(1, 1, 7, "t0")
    r.pub(1, 1, 2, exchange="dlx", key="")
    r.end(3)
    w = r.want[2]
    assert w["counters"]["n_dl_cycle"] == 40 and len(got(w, 0)) == 40 + 3 + 7 + 2
    assert w["depth"][r.q["src"]["slot"]] == 3 + 2
    return r


def sc_ban_counts(dp, n):
    """n banned names given by a client-supplied array over 64 declared queues behind a fanout, plus
    names that match no queue (ignored).  The source queue itself is not bound."""
    r = XRec(dp, TTL_STEP)
    r.exchange("dlx", "fanout")
    r.open(1)
    for i in range(64):
        r.queue(f"old{i}")
        r.bind(f"old{i}", "dlx")
    r.queue("src", dlx="dlx")
    arr = [element(i) for i in range(n - 1)] + [dict(element(0), queue="nowhere")] * (1 if n < 63 else 0)
    arr += [element(63, "rejected"), element(62)] if n < 62 else []
    r.pub(1, 1, 1, "src", expire_ms=1000, props={"headers": {"x-death": arr}})
    r.end(4)
    c = r.want[3]["counters"]
    assert c["n_dl_cycle"] == n - 1 and sum(r.want[3]["depth"].values()) == 64 - (n - 1), (c, n)
    return r


def sc_durable(dp):
    """A persisting plane: the store record of the dead letter carries the new property bytes."""
    r = XRec(dp, TTL_STEP, persist_budget=1280)
    r.exchange("dlx", "fanout")
    r.queue("park", durable=True)
    r.bind("park", "dlx")
    r.queue("src", durable=True, dlx="dlx")
    r.open(1)
    r.pub(1, 1, 2, "src", expire_ms=1000, props={"delivery_mode": 2, "headers": {"a": 1}})
    r.end(3)
    r.consume(2, 1, "park", later=True)
    r.end(2)
    st = r.want[3]["stored"]
    assert len(st) == 2 and all(b"x-death" in x[4] and b"x-first-death-queue" in x[4] for x in st)
    return r


BIG = dict(q_max=128, cons_max=512)
SCENARIOS = {
    "first_death": Scenario(sc_first_death, dict(queue_limits=True), TTL_STEP, True),
    "recount": Scenario(sc_recount, {}, TTL_STEP, False),
    "recount_mixed": Scenario(sc_recount_mixed, {}, TTL_STEP, False),
    "names": Scenario(sc_names, {}, TTL_STEP, True),
    "client_arrays": Scenario(sc_client_arrays, {}, TTL_STEP, True),
    "size_bound": Scenario(sc_size_bound, {}, TTL_STEP, True),
    "prefix": Scenario(sc_prefix, dict(dead_bytes=prefix_bytes()), TTL_STEP, True),
    "cycles": Scenario(sc_cycles, {}, TTL_STEP, False),
    "ban_direct": Scenario(sc_ban_direct, {}, TTL_STEP, True),
    "ban_fanout": Scenario(sc_ban_fanout, {}, TTL_STEP, True),
    "ban_topic": Scenario(sc_ban_topic, {}, TTL_STEP, True),
    "ban_hop": Scenario(sc_ban_hop, {}, TTL_STEP, True),
    "ban_headers": Scenario(sc_ban_headers, dict(headers_match=True), TTL_STEP, True),
    "ban_many": Scenario(sc_ban_many, {}, TTL_STEP, False),
    "ban_1": Scenario(lambda dp: sc_ban_counts(dp, 1), BIG, TTL_STEP, False),
    "ban_63": Scenario(lambda dp: sc_ban_counts(dp, 63), BIG, TTL_STEP, False),
    "ban_64": Scenario(lambda dp: sc_ban_counts(dp, 64), BIG, TTL_STEP, False),
    "durable": Scenario(sc_durable, PERSIST_CFG, TTL_STEP, True),
}
