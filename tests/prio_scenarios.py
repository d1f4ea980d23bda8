"""Priority queues (x-max-priority, ``priority_queues=True``) in the ``bytelimit_scenarios`` style:
each scenario is ``(dp, on) -> PRec`` with its own engine overrides on top of ``gpu_cfg.CFG``.

``PRec`` is the scenarios' own record: for every queue one plain Python list per priority (an
ordinary queue: one list), to which it applies the rule as CHANGES.md "Priority queues on the GPU
path" states it.

* A message's priority is the ``priority`` octet of its properties, 0 when absent (or when the
  property list is cut short), P when above P.
* Among a queue's ready messages the highest priority goes first, to Basic.Get and to consumers;
  within one priority the order is FIFO.  A requeued message returns to the front of its own
  priority.  Expiry is looked at at the head of each priority.
* Consumers share what is ready by the dispatch's credit rule: in round-robin order from the
  queue's cursor, consumer j of m takes min(ceil(remaining / (m - j)), its prefetch credit, the
  channel's window room); at most 64 runs a queue a step, the Get answers among them.
* On one channel the step's deliveries come queue by queue in slot order; within a priority queue
  priority by priority, highest first; within one priority the Get answers, then the consumers'
  pieces in round-robin order.

While a scenario is written the record builds the wire input of every step and predicts what the
step must put on the wire, the depth it leaves per priority and the step's counters.  It never
looks at the golden model: ``check`` judges the golden model's run and the HIP data plane's alike.
"""

import struct
from collections import defaultdict, namedtuple

from chanamq_amd.engine.traffic import ack_frame, publish_command
from chanamq_amd.protocol.codec import FrameParser, Method, decode_method, encode_frame, encode_method_frame, encode_properties, render_command
from consumer_scenarios import GOLDEN_KEYS, body_of, nack
from dp_scenarios import NOW, VH, get_cmd
from limit_scenarios import TWO_PASS

Scenario = namedtuple("Scenario", "fn cfg now_step_ms drained")
COUNTERS = ("n_deliv", "n_expired", "n_requeue", "n_ring_full", "n_unroutable")
DL_COUNTERS = ("n_dl_expired", "n_dl_rejected", "n_dl_cycle", "n_dl_unrouted")
DELIVER_CAP = 4096     # gpu_cfg.CFG deliver_cap
RUNS_PER_Q = 64        # dp_state.h
SORT_TILE = 1024       # dp_state.h
PUB_QC = 8             # dp_state.h
PRIO_MAX = 15          # prio_plan.h


class Entry:
    __slots__ = ("body", "expire", "red", "seq", "prio", "wire")

    def __init__(self, body, expire, seq, prio, wire=None):
        self.body, self.expire, self.red, self.seq, self.prio = body, expire, False, seq, prio
        self.wire = wire   # exchange + routing key + property + body bytes (None: not sized here)


def raw_publish(ch, exchange, key, body, props_bytes):
    """A Basic.Publish whose property list is the given bytes, whatever they are."""
    m = encode_method_frame(ch, Method("basic.publish", exchange=exchange, routing_key=key, mandatory=False))
    hdr = struct.pack(">HHQ", 60, 0, len(body)) + props_bytes
    return m + encode_frame(2, ch, hdr) + (encode_frame(3, ch, body) if body else b"")


def reject_frame(ch, tag, requeue=False):
    return render_command(ch, Method("basic.reject", delivery_tag=tag, requeue=requeue))


class PRec:
    """The record.  Topology calls go to the plane at once; traffic calls collect the current
    step, ``end`` closes it.  ``on``: the priority flag of the plane the scenario is written for."""

    def __init__(self, dp, on=True, now_step_ms=0, ucap=256, dl=False):
        self.dp, self.on, self.now_step_ms, self.ucap, self.dl = dp, on, now_step_ms, ucap, dl
        self.q = {}                       # name -> dict(slot, P, lanes, ttl, cons, rr, dlq, dl_self)
        self.chan = {}                    # (conn, ch) -> dict(tag, unacked, prefetch, global_, win)
        self.fan = defaultdict(list)
        self.steps, self.want = [], []
        self.seq = 0
        # what bounds a step's deliveries, where a scenario sets it (None: it does not bind):
        # deliver-cap-bytes, the step's egress byte budget, its delivery slots, its pair table
        self.dcap = self.egress_cap = self.deliv_max = self.pair_max = None
        self.waiting = defaultdict(list)  # (queue, lane) -> requeued entries its ring had no room for
        self.dead = []                    # dead letters awaiting the next step's pass: (target queue, entry props' priority, body)
        self._new_step()

    def _new_step(self):
        self.cur = defaultdict(bytes)
        self.ops, self.pubs, self.settles, self.gets, self.rejects = [], [], [], [], []

    # ---- topology
    def queue(self, name, P=None, ttl=0, cap=None, keep=None, dlq=None, dl_self=False, later=False, slot=None):
        """``P``: x-max-priority (None: an ordinary queue); ``cap``: rings of exactly that many
        slots that cannot grow; ``keep``: rings of that many slots that may; ``dlq``: the queue the
        dead-letter exchange (amq.fanout) feeds; ``dl_self``: the dead-letter exchange is the default
        exchange with the queue's own name as the key."""
        kw = dict(ttl_ms=ttl)
        if P is not None:
            kw["max_priority"] = P
        if cap:
            kw.update(capacity=cap, max_capacity=cap)
        if keep:
            kw.update(capacity=keep)
        if dlq:
            kw["dead_letter_exchange"] = "amq.fanout"
        if dl_self:
            kw.update(dead_letter_exchange="", dead_letter_routing_key=name)
        if later:
            self.ops.append(("declare_queue", (VH, name), kw))
        else:
            slot = self.dp.declare_queue(VH, name, **kw)
        eff = P if self.on else None
        self.q[name] = dict(slot=slot, P=eff, lanes=[[] for _ in range((eff or 0) + 1)], ttl=ttl, cons=[], rr=0,
                            cap=cap, dlq=dlq, dl_self=dl_self, serial=0)
        return slot

    def delete(self, name):
        self.ops.append(("delete_queue", (VH, name)))
        return self.q.pop(name)["slot"]

    def purge(self, name):
        self.ops.append(("purge", (self.q[name]["slot"],)))
        for lane in self.q[name]["lanes"]:
            for e in lane:
                e.expire = 1

    def open(self, conn, ch=1, prefetch=0, global_=False):
        if not any(c == conn for c, _ in self.chan):
            self.dp.open_connection(conn, VH)
        self.dp.open_channel(conn, ch)
        if prefetch:
            self.dp.qos(conn, ch, prefetch, 0, global_)
        self.chan[(conn, ch)] = dict(tag=0, unacked=[], prefetch=prefetch, global_=global_, win=[])

    def bind_fanout(self, q, exchange="amq.fanout"):
        self.dp.bind(VH, q, exchange, "")
        self.fan[exchange].append(q)

    def consume(self, conn, ch, q, no_ack=True, tag=None, later=False):
        tag = tag or "c-%s-%d-%d" % (q, conn, ch)
        call = ("consume", (conn, ch, VH, q, tag), dict(no_ack=no_ack))
        if later:
            self.ops.append(call)
        else:
            self.dp.consume(*call[1], **call[2])
        self.q[q]["cons"].append(dict(conn=conn, ch=ch, tag=tag, no_ack=no_ack))

    # ---- the current step
    def pub(self, conn, ch, prios, q=None, exchange="", size=0, expire_ms=0, extra=None, raw=None):
        """One publish per entry of ``prios`` (None: no priority property) to queue ``q`` through the
        default exchange, or to a fanout exchange.  ``extra``: further properties; ``raw``:
        ``(property bytes, the priority they mean)`` instead."""
        name = q if q is not None else exchange
        for pr in prios:
            if q is not None:
                i, self.q[q]["serial"] = self.q[q]["serial"], self.q[q]["serial"] + 1
            else:
                i = self.seq
            body = body_of(name, i, size)
            if raw is not None:
                pb, pr = raw
                self.cur[conn] += raw_publish(ch, exchange, q or "", body, pb)
            else:
                p = dict(extra or {})
                if pr is not None:
                    p["priority"] = pr
                if expire_ms:
                    p["expiration"] = str(expire_ms)
                self.cur[conn] += publish_command(ch, exchange, q or "", body, p or None)
            plen = len(pb) if raw is not None else len(encode_properties(p))
            self.pubs.append((conn, len(self.pubs), ch, [q] if q is not None else sorted(self.fan[exchange]), body,
                              expire_ms, pr or 0, len(exchange) + len(q or "") + plen + len(body)))
            self.seq += 1

    def ack_all(self, conn, ch):
        self.cur[conn] += ack_frame(ch, 0, multiple=True)
        self.settles.append((conn, ch, False))

    def nack_all(self, conn, ch):
        self.cur[conn] += nack(ch, 0)
        self.settles.append((conn, ch, True))

    def recover(self, conn, ch):
        self.ops.append(("recover", (conn, ch)))
        self.settles.append((conn, ch, True))

    def reject_all(self, conn, ch):
        """Basic.Reject without requeue of every unacked delivery of the channel."""
        for qn, li, e, tag, _ in self.chan[(conn, ch)]["unacked"]:
            self.cur[conn] += reject_frame(ch, tag)
        self.rejects.append((conn, ch))

    def cap_bytes(self, n):
        """deliver-cap-bytes from this step on: a consumer whose share is more than one entry takes at
        most max(1, n // s) a step, s the rendered size of the first entry it would get."""
        self.ops.append(("set_deliver_cap_bytes", (n,)))
        self.dcap = n

    @staticmethod
    def deliver_size(c, e):
        """Rendered bytes of a Basic.Deliver of ``e`` to consumer ``c``: method, header and one body
        frame (8 bytes of framing each) around the consumer tag, delivery tag, flags, exchange,
        routing key, the 12 header bytes, the properties and the body."""
        return 52 + len(c["tag"]) + e.wire

    def get(self, conn, ch, q, n=1):
        self.cur[conn] += get_cmd(ch, q, True) * n
        self.gets += [(conn, ch, q)] * n

    # ---- the rules
    def end(self, n=1):
        for _ in range(n):
            self._end()

    @staticmethod
    def lane_index(q, prio):
        return 0 if q["P"] is None else q["P"] - min(prio, q["P"])

    def _end(self):
        k = len(self.steps)
        now = NOW + self.now_step_ms * k
        cnt = dict.fromkeys(COUNTERS + (DL_COUNTERS if self.dl else ()), 0)
        empty = defaultdict(int)
        for c in self.chan.values():
            c["win"] = [s for s in c["win"] if s in [id(u[2]) for u in c["unacked"]]]
        # (1) enqueue in publish order (connection, then wire order), the dead letters of the last
        # step behind them: each pair to the list of its message's priority
        # (a full pair table: a publish's pairs stand in queue-slot order behind the earlier publishes';
        # those past pair_max are dropped and counted as n_ring_full)
        arrivals, npairs = [], 0
        for conn, _, ch, qs, body, exp_ms, pr, wire in sorted(self.pubs, key=lambda p: p[:2]):
            if not qs:
                cnt["n_unroutable"] += 1
            for qn in sorted(qs, key=lambda n: self.q[n]["slot"]):
                npairs += 1
                if self.pair_max is not None and npairs > self.pair_max:
                    cnt["n_ring_full"] += 1
                    continue
                arrivals.append((qn, body, exp_ms, pr, wire))
        # (the dead pass takes the list by source slot, then position: deaths of one slot are in that order)
        for _, qn, pr, body, banned in sorted(self.dead, key=lambda d: d[0]):
            if banned:
                cnt["n_dl_cycle"] += 1
                cnt["n_dl_unrouted"] += 1
            else:
                arrivals.append((qn, body, 0, pr, None))
        self.dead = []
        for qn, body, exp_ms, pr, wire in arrivals:
            q = self.q[qn]
            lane = q["lanes"][self.lane_index(q, pr)]
            if q["cap"] and len(lane) >= q["cap"]:
                cnt["n_ring_full"] += 1
                continue
            exp = [e for e in (now + exp_ms if exp_ms else 0, now + q["ttl"] if q["ttl"] else 0) if e]
            lane.append(Entry(body, min(exp) if exp else 0, self.seq, pr, wire))
            self.seq += 1
        # (2) settles: rejects die (dead-lettered where the queue says so), requeues go back in
        # front of their own priority, in their first order; a ring without room keeps them waiting
        for conn, ch in self.rejects:
            c = self.chan[(conn, ch)]
            for qn, li, e, tag, _ in c["unacked"]:
                self._dies(cnt, qn, li, e, "n_dl_rejected")
            c["unacked"], c["win"] = [], []
        back = defaultdict(list)
        for conn, ch, requeue in self.settles:
            c = self.chan[(conn, ch)]
            for qn, li, e, tag, _ in c["unacked"]:
                if requeue:
                    back[(qn, li)].append(e)
                    cnt["n_requeue"] += 1
            c["unacked"], c["win"] = [], []
        for key in sorted(set(back) | {k for k, w in self.waiting.items() if w}):
            qn, li = key
            for e in back.get(key, ()):
                e.red = True
            q = self.q[qn]
            lane = q["lanes"][li]
            # those waiting and the new ones in their first order; what the ring has room for goes
            # in front of the head, the rest waits for a later step
            es = sorted(self.waiting[key] + back.get(key, []), key=lambda e: e.seq)
            k = len(es) if not q["cap"] else max(min(len(es), q["cap"] - len(lane)), 0)
            lane[:0] = es[:k]
            self.waiting[key] = es[k:]
        # (3) per queue in slot order: expiry at the head of each priority, Basic.Gets, dispatch
        egress_used = deliv_used = 0   # the step's egress bytes and delivery slots reserved so far
        runs = []   # (lane slot, order, conn, ch, kind, consumer tag, queue, lane index, entry, no_ack)
        for qn, q in sorted(self.q.items(), key=lambda kv: kv[1]["slot"]):
            for li, lane in enumerate(q["lanes"]):
                while lane and lane[0].expire and lane[0].expire <= now:
                    e = lane.pop(0)
                    cnt["n_expired"] += 1
                    if e.expire != 1:
                        self._dies(cnt, qn, li, e, "n_dl_expired")
            nget = 0
            for conn, ch, gq in self.gets:
                if gq != qn:
                    continue
                li = next((i for i, lane in enumerate(q["lanes"]) if lane), None)
                if li is None:
                    empty[(conn, ch)] += 1
                    continue
                assert nget < RUNS_PER_Q // 2, "scenario: at most 32 Gets a queue a step"
                assert self.egress_cap is None and self.deliv_max is None, "scenario: no Gets beside a step cut"
                runs.append((q["slot"] + li, len(runs), conn, ch, "get_ok", None, qn, li, q["lanes"][li].pop(0), True))
                nget += 1
            v = [(li, e) for li, lane in enumerate(q["lanes"]) for e in lane]
            mall = len(q["cons"])
            if not mall or not v:
                continue
            m = min(mall, RUNS_PER_Q - nget)
            remaining, off = len(v), 0
            grants = []
            pending = defaultdict(int)   # (channel) -> granted in this queue's step, not yet delivered
            for j in range(m):
                c = q["cons"][(q["rr"] + j) % mall]
                chan = self.chan[(c["conn"], c["ch"])]
                key = (c["conn"], c["ch"])
                g = 0
                if remaining:
                    g = min(-(-remaining // (m - j)), DELIVER_CAP)
                    if self.dcap and g > 1:   # by the first entry the consumer would get
                        s0 = self.deliver_size(c, v[off][1])
                        g = min(g, 1 if s0 >= self.dcap else self.dcap // s0)
                    if not c["no_ack"] and chan["prefetch"]:
                        used = len(chan["unacked"]) + pending[key] if chan["global_"] else \
                            sum(1 for u in chan["unacked"] if u[4] is c)
                        g = min(g, max(chan["prefetch"] - used, 0))
                    g = min(g, self.ucap - len(chan["win"]) - pending[key])
                grants.append([c, g])
                pending[key] += g
                off += g
                remaining -= g
            # the egress budget: the longest prefix of the granted entries, in run order, whose frames fit
            if self.egress_cap is not None:
                sizes, pos = [], 0
                for c, g in grants:
                    sizes += [self.deliver_size(c, e) for _, e in v[pos:pos + g]]
                    pos += g
                left = max(self.egress_cap - egress_used, 0)
                egress_used += sum(sizes)
                if sum(sizes) > left:
                    keep = 0
                    while keep < len(sizes) and sizes[keep] <= left:
                        left -= sizes[keep]
                        keep += 1
                    for gr in grants:
                        gr[1], keep = min(gr[1], keep), keep - min(gr[1], keep)
            # the delivery slots: what is over goes from the last run backwards
            if self.deliv_max is not None:
                total = sum(g for _, g in grants)
                excess = total - min(total, max(self.deliv_max - deliv_used, 0))
                deliv_used += total
                for gr in reversed(grants):
                    take = min(gr[1], excess)
                    gr[1] -= take
                    excess -= take
            off = 0
            for c, g in grants:
                chan = self.chan[(c["conn"], c["ch"])]
                for li, e in v[off:off + g]:
                    q["lanes"][li].remove(e)
                    self._deliver(c, chan, e, qn, li)
                    runs.append((q["slot"] + li, len(runs), c["conn"], c["ch"], "deliver", c["tag"], qn, li, e, c["no_ack"]))
                off += g
            q["rr"] = (q["rr"] + 1) % mall
        # tags: per channel, its runs by lane slot, then in the order they were made
        ev = defaultdict(list)
        for slot, _, conn, ch, kind, ctag, qn, li, e, no_ack in sorted(runs, key=lambda r: r[:2]):
            chan = self.chan[(conn, ch)]
            chan["tag"] += 1
            if kind == "get_ok":
                chan["win"].append(id(e))
            for u in chan["unacked"]:
                if u[2] is e:
                    u[3] = chan["tag"]
            ev[(conn, ch)].append((kind, ctag, e.body, e.red, chan["tag"]))
            cnt["n_deliv"] += 1
        inp = {c: b for c, b in self.cur.items()}
        if self.ops:
            inp["__ops__"] = self.ops
        self.steps.append(inp)
        self.want.append(dict(events=dict(ev), empty=dict(empty), confirms={}, counters=cnt,
                              depth={q["slot"] + li: len(lane) for q in self.q.values() for li, lane in enumerate(q["lanes"])}))
        self._new_step()

    def _deliver(self, c, chan, e, qn, li):
        chan["win"].append(id(e))
        assert len(chan["win"]) <= self.ucap
        if not c["no_ack"]:
            chan["unacked"].append([qn, li, e, 0, c])

    def _dies(self, cnt, qn, li, e, counter):
        q = self.q[qn]
        if q["dlq"]:
            cnt[counter] += 1
            self.dead.append((q["slot"] + li, q["dlq"], e.prio, e.body, False))
        elif q["dl_self"]:
            cnt[counter] += 1
            # back to the queue itself: with x-death on, an expiry is a cycle (the queue's own name
            # stands in the history) and the dead letter is lost; a rejection may go round
            self.dead.append((q["slot"] + li, qn, e.prio, e.body, counter == "n_dl_expired"))


# ---------------------------------------------------------------- planes and runner
DL_CFG = dict(dead_letter=True, dead_max=1024, dead_bytes=1 << 20)
XD_CFG = dict(DL_CFG, x_death=True)
DL_KEYS = ("dead_max", "dead_bytes", "restore_max")


def cfg_of(sc, base):
    return dict(base, **sc.cfg)


def plane_kw(cfg, on):
    kw = {}
    if on:
        kw["priority_queues"] = True
    for k in ("dead_letter", "x_death"):
        if cfg.get(k):
            kw[k] = True
    return kw


def golden_plane(cfg, on=True):
    from chanamq_amd.engine.golden import GoldenDataPlane
    kw = {k: cfg[k] for k in GOLDEN_KEYS + ("ring_pool", "deliv_max", "egress_cap") + DL_KEYS if k in cfg}
    return GoldenDataPlane(**kw, **plane_kw(cfg, on))


def gpu_plane(cfg, graph, on=True):
    from chanamq_amd.engine.dataplane import GpuDataPlane
    return GpuDataPlane(graph=graph, **dict(cfg, **plane_kw(cfg, on)))


def slot_depth(dp, s):
    """Ready entries of slot ``s`` alone (a lane, not the queue's sum)."""
    if hasattr(dp, "eng"):
        return dp._u64("q_tail", s) - dp._u64("q_head", s)
    return len(dp.ring[s])


def slot_capacity(dp, q):
    if hasattr(dp, "eng"):
        return dp._u64("q_ring_mask", q.slot) + 1
    return q.capacity


def run_prio(dp, rec):
    """Drive dp through the record's steps (control ops first, the clock advanced per step): the
    egress, the counters, the depth and ring capacity of every slot in use, lanes included."""
    outs = []
    names = COUNTERS + (DL_COUNTERS if rec.dl else ())
    for k, inp in enumerate(rec.steps):
        inp = dict(inp)
        res = []
        for op in inp.pop("__ops__", []):
            res.append(getattr(dp, op[0])(*op[1], **(op[2] if len(op) > 2 else {})))
        r = dp.step(inp, now_ms=NOW + rec.now_step_ms * k)
        if isinstance(r, dict):
            eg, ctrl, ev, cnt = r["egress"], r["ctrl"], r["events"], r["counters"]
        else:
            eg, ctrl, ev, cnt = r.egress, r.ctrl, r.events, r.counters
        outs.append(dict(egress=eg, ctrl=sorted(ctrl), events=sorted(ev), gets=[], txbuf=[], segs=[],
                         ops=[x for x in res if isinstance(x, tuple)],
                         counters={c: int(cnt.get(c, 0)) for c in names},
                         depth={s: int(slot_depth(dp, s)) for s in sorted(dp.queue_by_slot)},
                         cap={s: int(slot_capacity(dp, q)) for s, q in sorted(dp.queue_by_slot.items())}))
    return outs


def observe(out, k):
    """One step's egress as the record states it (``limit_scenarios.observe``, but the content header
    is read for its body size alone: some property lists here are cut short on purpose)."""
    ev, empty = defaultdict(list), defaultdict(int)
    for conn in sorted(out["egress"]):
        fp, cur = FrameParser(), None
        for fr in fp.feed(out["egress"][conn]):
            if fr.type == 1:
                assert cur is None, f"step {k} conn {conn}: method frame inside content"
                m = decode_method(fr.payload)
                if m.name == "basic.get_empty":
                    empty[(conn, fr.channel)] += 1
                else:
                    assert m.name in ("basic.deliver", "basic.get_ok"), f"step {k} conn {conn}: unexpected {m.name}"
                    cur = [fr.channel, m, None, []]
                continue
            assert cur is not None and fr.channel == cur[0], f"step {k} conn {conn}: stray content frame"
            if fr.type == 2:
                cur[2] = struct.unpack_from(">Q", fr.payload, 4)[0]
            else:
                cur[3].append(fr.payload)
            if cur[2] is not None and sum(map(len, cur[3])) >= cur[2]:
                m, get = cur[1], cur[1].name == "basic.get_ok"
                ev[(conn, cur[0])].append(("get_ok" if get else "deliver", None if get else m.consumer_tag, b"".join(cur[3]),
                                           bool(m.redelivered), m.delivery_tag))
                cur = None
        assert cur is None and not fp.buf, f"step {k} conn {conn}: egress ends inside a command"
    return dict(ev), dict(empty), {}


def check(rec, outs):
    """The run against the record, step by step."""
    assert len(outs) == len(rec.want)
    for k, (o, w) in enumerate(zip(outs, rec.want)):
        ev, empty, conf = observe(o, k)
        short = lambda d: {c: [(e[0], e[2], e[3], e[4]) for e in v] for c, v in d.items()}
        assert ev == w["events"], f"step {k}: deliveries differ: got {short(ev)}, expected {short(w['events'])}"
        assert empty == w["empty"], f"step {k}: GetEmpty {empty}, expected {w['empty']}"
        assert o["counters"] == w["counters"], f"step {k}: counters {o['counters']}, expected {w['counters']}"
        assert o["depth"] == w["depth"], f"step {k}: depths {o['depth']}, expected {w['depth']}"


def compare(og, od):
    """Two planes' runs, step by step: egress bytes, counters, depths per lane, ring capacities."""
    assert len(og) == len(od)
    for k, (a, b) in enumerate(zip(og, od)):
        assert a["egress"] == b["egress"], f"step {k}: egress bytes differ"
        assert a["ctrl"] == b["ctrl"] and a["events"] == b["events"], f"step {k}"
        assert a["ops"] == b["ops"], f"step {k}: control results differ"
        assert a["counters"] == b["counters"], f"step {k}: {a['counters']} / {b['counters']}"
        assert a["depth"] == b["depth"], f"step {k}: depths differ"
        assert a["cap"] == b["cap"], f"step {k}: ring capacities differ"


# ---------------------------------------------------------------- scenarios
def sc_order_basic(dp, on=True):
    """P = 3; priorities 0..3, 4, 255 and none are published before a consumer attaches: highest
    first, FIFO within one priority (4 and 255 count as 3, none as 0)."""
    r = PRec(dp, on)
    r.queue("ob", P=3)
    r.open(1)
    r.open(2)
    r.pub(1, 1, [0, 1, 2, 3, 4, 255, None, 2, 0, 3, 1], q="ob")
    r.end()
    r.pub(1, 1, [1, 3], q="ob")
    r.consume(2, 1, "ob", later=True)
    r.end()
    r.pub(1, 1, [0, 2, 0, 3], q="ob")
    r.end(2)
    return r


def sc_props_shapes(dp, on=True):
    """The priority behind content-type, content-encoding, a headers table and delivery-mode; with
    none of them; behind a two-word flags chain; a list cut inside the priority octet (0); a list
    cut behind it (no properties at all: 0).  P = 1 and P = 15."""
    r = PRec(dp, on)
    r.queue("p1", P=1)
    r.queue("p15", P=PRIO_MAX)
    r.open(1)
    r.open(2)
    shapes = [dict(content_type="text/plain"), dict(content_encoding="gzip"), dict(headers={"k": "v", "n": 7}),
              dict(delivery_mode=1), dict(content_type="a", content_encoding="b", headers={"x": "y"}, delivery_mode=2),
              dict(message_id="m", timestamp=1_700_000_000, app_id="app")]
    for qn, top in (("p1", 1), ("p15", PRIO_MAX)):
        r.pub(1, 1, [0], q=qn)
        for i, extra in enumerate(shapes):
            r.pub(1, 1, [1 + (i * 5) % top], q=qn, extra=extra)
        r.pub(1, 1, [top], q=qn)
        full = encode_properties(dict(content_type="ct", priority=top))
        two = bytes([full[0], full[1] | 1, 0, 0]) + full[2:]          # a continuation word without fields
        r.pub(1, 1, [None], q=qn, raw=(two, top))
        r.pub(1, 1, [None], q=qn, raw=(full[:-1], 0))                 # cut inside the priority octet
        late = encode_properties(dict(priority=top, message_id="abcdef"))
        r.pub(1, 1, [None], q=qn, raw=(late[:-2], 0))                 # cut behind it, inside message-id
        r.pub(1, 1, [None], q=qn, raw=(two[:2], 0))                   # cut inside the flags chain
    r.end()
    r.consume(2, 1, "p1", later=True)
    r.consume(2, 1, "p15", later=True)
    r.end(2)
    return r


def sc_lane_pairs(dp, on=True):
    """Pair counts around a wave multiple and a sort tile; a fanout to an ordinary queue and two
    priority queues with different P (only their pairs move); more than PUB_QC queues a publish."""
    r = PRec(dp, on)
    r.queue("plain")
    r.queue("pa", P=2)
    r.queue("pb", P=5)
    for qn in ("plain", "pa", "pb"):
        r.bind_fanout(qn)
    dp.declare_exchange(VH, "wide.fan", "fanout")
    many = ["m%d" % i for i in range(PUB_QC + 2)]
    for i, qn in enumerate(many):
        r.queue(qn, P=(1 + i % 3) if i % 2 else None)
        r.bind_fanout(qn, "wide.fan")
    r.open(1)
    r.open(2)
    for n in (255, 256, 257, SORT_TILE - 1, SORT_TILE, SORT_TILE + 1):   # pairs of the step
        r.pub(1, 1, [i % 7 for i in range(n // 3)], exchange="amq.fanout")
        r.pub(1, 1, [5 - i for i in range(n % 3)], q="pb")
        r.end()
    r.pub(1, 1, [3, 0, 1, 2], exchange="wide.fan")
    r.end()
    for i, qn in enumerate(["plain", "pa", "pb"] + many):
        if i < 8:
            r.open(2, 2 + i) if i < 7 else None
        r.consume(2, 1 + min(i, 7), qn, later=True)
    r.end(8)
    return r


def sc_span_lanes(dp, on=True):
    """One consumer whose grant covers three lanes (three runs in priority order on its channel);
    two priority queues and an ordinary queue consumed on one channel."""
    r = PRec(dp, on)
    r.queue("s1", P=2)
    r.queue("mid")
    r.queue("s2", P=4)
    r.open(1)
    r.open(2)
    r.pub(1, 1, [0, 1, 2, 0, 1, 2], q="s1")
    r.pub(1, 1, [None] * 3, q="mid")
    r.pub(1, 1, [4, 0, 2, 9], q="s2")
    r.end()
    for qn in ("s2", "mid", "s1"):
        r.consume(2, 1, qn, later=True)
    r.end(2)
    return r


def sc_credit_cuts(dp, on=True):
    """Prefetch 1; a prefetch that ends inside a lane; a global prefetch shared by two consumers of
    one channel: the grant is a prefix of V, the rest stays in its lanes."""
    r = PRec(dp, on)
    r.queue("c1", P=3)
    r.queue("c2", P=2)
    r.queue("c3", P=2)
    r.open(1)
    r.open(2, 1, prefetch=1)
    r.open(2, 2, prefetch=5)
    r.open(3, 1, prefetch=4, global_=True)
    r.pub(1, 1, [1, 3, 0, 3, 2], q="c1")
    r.pub(1, 1, [2, 2, 2, 1, 1, 1, 1, 0], q="c2")
    r.pub(1, 1, [0, 1, 2, 2, 1, 0], q="c3")
    r.end()
    r.consume(2, 1, "c1", no_ack=False, later=True)
    r.consume(2, 2, "c2", no_ack=False, later=True)
    r.consume(3, 1, "c3", no_ack=False, tag="g-a", later=True)
    r.consume(3, 1, "c3", no_ack=False, tag="g-b", later=True)
    r.end()
    for _ in range(3):
        r.ack_all(2, 1)
        r.end()
    r.pub(1, 1, [3], q="c1")     # a newcomer of the highest priority overtakes what waits
    r.ack_all(2, 1)
    r.ack_all(2, 2)
    r.ack_all(3, 1)
    r.end()
    for _ in range(3):
        r.ack_all(2, 1)
        r.ack_all(2, 2)
        r.ack_all(3, 1)
        r.end()
    return r


def sc_cap_bytes(dp, on=True):
    """deliver-cap-bytes: each consumer takes what fits the cap by the size of the first entry it
    would get -- for the second consumer an entry inside a lower lane -- and one entry when that
    alone is over the cap."""
    r = PRec(dp, on)
    r.queue("cb", P=2)
    r.open(1)
    r.open(2)
    r.open(3)
    r.pub(1, 1, [2, 2], q="cb", size=100)
    r.pub(1, 1, [1, 1, 1], q="cb", size=300)
    r.pub(1, 1, [0] * 6, q="cb", size=100)
    r.end()
    r.cap_bytes(700)
    r.consume(2, 1, "cb", later=True)
    r.consume(3, 1, "cb", later=True)
    r.end(2)
    r.cap_bytes(120)      # below one delivery: one entry a consumer a step
    r.end()
    r.cap_bytes(0)
    r.end(2)
    return r


def cut_fill(r, name="cq"):
    """A queue of three lanes x five entries of 100 bytes and two consumers on channels of their own."""
    r.queue(name, P=2)
    r.open(1)
    r.open(2)
    r.open(3)
    r.pub(1, 1, [i % 3 for i in range(15)], q=name, size=100)
    r.end()
    r.consume(2, 1, name, later=True)
    r.consume(3, 1, name, later=True)


BUDGET_CFG = dict(egress_cap=2048)


def sc_budget_cut(dp, on=True):
    """The step's egress budget ends inside a lane: of the two consumers' pieces the longest prefix
    of V whose frames fit is delivered, the rest stays in its lanes for the next steps."""
    r = PRec(dp, on)
    r.egress_cap = BUDGET_CFG["egress_cap"]
    cut_fill(r)
    r.end(3)
    return r


SLOT_CFG = dict(deliv_max=8)


def sc_slot_cut(dp, on=True):
    """deliv_max ends inside a lane: the grants are trimmed from the last run backwards, across
    lanes, so the first consumer keeps its piece and V's tail stays queued."""
    r = PRec(dp, on)
    r.deliv_max = SLOT_CFG["deliv_max"]
    cut_fill(r)
    r.end(3)
    return r


PAIR_CFG = dict(pair_max=64)


def sc_pair_cut(dp, on=True):
    """A publish the full pair table cuts short: a fanout to a priority queue, an ordinary queue and
    another priority queue, three pairs a publish into a table of 64.  The 22nd publish keeps its
    pair for the lowest slot -- a priority queue's base, moved to its lane like any other -- and
    loses two; the 23rd loses all three."""
    r = PRec(dp, on)
    r.pair_max = PAIR_CFG["pair_max"]
    r.queue("pa", P=2)
    r.queue("plain")
    r.queue("pb", P=5)
    for qn in ("pa", "plain", "pb"):
        r.bind_fanout(qn)
    r.open(1)
    r.open(2)
    r.pub(1, 1, [(i * 3 + 2) % 7 for i in range(23)], exchange="amq.fanout")
    r.end()
    r.pub(1, 1, [1, 5], exchange="amq.fanout")     # the next step's table has room again
    for qn in ("pa", "plain", "pb"):
        r.consume(2, 1, qn, later=True)
    r.end(2)
    return r


MANY_CFG = dict(c_max=128, cons_max=256)


def sc_many_consumers(dp, on=True):
    """RUNS_PER_Q and RUNS_PER_Q + 1 consumers, Gets taking run slots beside them, the round-robin
    cursor advancing: the window serves 64 runs a step, the Get answers among them."""
    r = PRec(dp, on)
    r.queue("mq", P=2)
    r.queue("mr", P=1)
    r.open(1)
    r.open(2)
    for c in range(RUNS_PER_Q + 1):
        r.open(10 + c)
        r.consume(10 + c, 1, "mq")
        if c < RUNS_PER_Q:
            r.consume(10 + c, 1, "mr")
    for _ in range(3):
        r.pub(1, 1, [i % 3 for i in range(150)], q="mq")
        r.pub(1, 1, [i % 2 for i in range(70)], q="mr")
        r.get(2, 1, "mq", 3)
        r.end()
    r.end(2)
    return r


def sc_gets(dp, on=True):
    """Gets with the top lane empty and a lower one not; an empty queue (GetEmpty); message counts
    over all lanes; Gets ahead of a consumer in one step."""
    r = PRec(dp, on)
    r.queue("g", P=3)
    r.queue("ge", P=2)
    r.open(1)
    r.open(2)
    r.open(3)
    r.open(4)
    r.pub(1, 1, [0, 2, 2, 1, 0], q="g")
    r.get(4, 1, "ge")
    r.end()
    r.get(2, 1, "g", 2)
    r.end()
    r.pub(1, 1, [3, 1], q="g")
    r.get(2, 1, "g", 2)
    r.get(4, 1, "ge")
    r.consume(3, 1, "g", later=True)
    r.end()
    r.get(2, 1, "g")
    r.end()
    return r


def sc_requeue(dp, on=True):
    """Nack-requeue and recover put entries back at the front of their own priority, ahead of the
    lower ones and behind nothing of a higher one; a newcomer of a higher priority still overtakes."""
    r = PRec(dp, on)
    r.queue("rq", P=2, keep=8)
    r.queue("rf", P=1, cap=4)       # rings of four slots that cannot grow
    r.open(1)
    r.open(2, 1, prefetch=4)
    r.open(3, 1, prefetch=3)
    r.pub(1, 1, [2, 1, 1, 0, 0, 2, 1], q="rq")
    r.consume(2, 1, "rq", no_ack=False, later=True)
    r.pub(1, 1, [1, 1, 1, 1], q="rf")
    r.consume(3, 1, "rf", no_ack=False, later=True)
    r.end()
    r.nack_all(2, 1)
    r.pub(1, 1, [2, 0], q="rq")
    # a lane ring without room: the step's enqueue fills the ring of priority 1 before the three
    # nacked entries come back, so they wait; the next step's head has room and takes them in front
    r.nack_all(3, 1)
    r.pub(1, 1, [1, 1, 1], q="rf")
    r.end()
    r.recover(2, 1)
    r.end()
    for _ in range(4):
        r.ack_all(2, 1)
        r.ack_all(3, 1)
        r.end()
    return r


TTL_STEP_MS = 600


def sc_ttl_dlx(dp, on=True):
    """Expired heads in several lanes in one step (an expired entry behind a live one of its own
    priority waits); x-message-ttl; a rejected message is dead-lettered; dead letters land on their
    own priority's lane of the target; with x-death on, a priority queue that dead-letters into
    itself by TTL ends empty with the cycle counted."""
    r = PRec(dp, on, now_step_ms=TTL_STEP_MS, dl=True)
    r.queue("tq", P=2, dlq="td")
    r.queue("td", P=3)
    r.bind_fanout("td")
    r.queue("tself", P=2, ttl=500, dl_self=True)
    r.queue("trej", P=1, dlq="td")
    r.open(1)
    r.open(2, 1, prefetch=3)
    r.open(3)
    r.pub(1, 1, [2, 2, 1, 0], q="tq", expire_ms=500)
    r.pub(1, 1, [2], q="tq")
    r.pub(1, 1, [2, 1], q="tq", expire_ms=500)        # behind a live one of priority 2: the 2 waits
    r.pub(1, 1, [0, 2, 1], q="tself")
    r.pub(1, 1, [1, 0, 1], q="trej")
    r.consume(2, 1, "trej", no_ack=False, later=True)
    r.end()
    r.reject_all(2, 1)
    r.end()
    r.end()
    r.consume(3, 1, "td", later=True)
    r.consume(3, 1, "tq", later=True)
    r.end(3)
    return r


GROW_CFG = dict(default_queue_capacity=1 << 12)


def sc_grow(dp, on=True):
    """A lane that grows twice and two lanes growing in one step; a lane ring that cannot grow
    refuses what does not fit (n_ring_full) while the other lanes take theirs."""
    r = PRec(dp, on)
    r.queue("gr", P=2, keep=4)
    r.queue("gf", P=1, cap=4)
    r.open(1)
    r.open(2)
    r.pub(1, 1, [2] * 6 + [1] * 8, q="gr")           # two lanes grow in one step (4 -> 16 each)
    r.pub(1, 1, [1] * 6 + [0] * 3, q="gf")           # lane 1 is full at 4, lane 0 takes its 3
    r.end()
    r.pub(1, 1, [2] * 14 + [0], q="gr")              # the top lane grows again (20 entries: 16 -> 64)
    r.end()
    r.consume(2, 1, "gr", later=True)
    r.consume(2, 1, "gf", later=True)
    r.end(2)
    return r


def sc_admin(dp, on=True):
    """Purge (every lane), delete and redeclare into the freed slots."""
    r = PRec(dp, on)
    r.queue("ad", P=2)
    r.queue("keep")
    r.open(1)
    r.open(2)
    r.pub(1, 1, [0, 1, 2, 2], q="ad")
    r.pub(1, 1, [None] * 2, q="keep")
    r.end()
    r.purge("ad")
    r.pub(1, 1, [1, 2], q="ad")      # behind the purge: they stay
    r.end()
    r.get(2, 1, "ad", 2)
    r.end()
    r.delete("ad")
    r.end()
    # (slots 0..2 went to the back of the free list: the next run of four is 4..7)
    r.queue("ad2", P=3, later=True, slot=4)
    r.pub(1, 1, [3, 0, 9], q="ad2")
    r.end()
    r.consume(2, 1, "keep", later=True)
    r.consume(2, 1, "ad2", later=True)
    r.end(2)
    return r


def sc_off(dp, on=False):
    """Flag off: x-max-priority is ignored, the queue is the FIFO it always was."""
    r = PRec(dp, False)
    r.queue("of", P=3)
    r.open(1)
    r.open(2)
    r.pub(1, 1, [0, 3, 1, 255, None, 2], q="of")
    r.get(2, 1, "of")
    r.end()
    r.consume(2, 1, "of", later=True)
    r.end(2)
    return r


SCENARIOS = {
    "order_basic": Scenario(sc_order_basic, {}, 0, True),
    "props_shapes": Scenario(sc_props_shapes, {}, 0, True),
    "lane_pairs": Scenario(sc_lane_pairs, {}, 0, True),
    "span_lanes": Scenario(sc_span_lanes, {}, 0, True),
    "credit_cuts": Scenario(sc_credit_cuts, {}, 0, True),
    "cap_bytes": Scenario(sc_cap_bytes, {}, 0, True),
    "many_consumers": Scenario(sc_many_consumers, MANY_CFG, 0, True),
    "gets": Scenario(sc_gets, {}, 0, False),
    "requeue": Scenario(sc_requeue, {}, 0, True),
    "ttl_dlx": Scenario(sc_ttl_dlx, XD_CFG, TTL_STEP_MS, False),
    "grow": Scenario(sc_grow, GROW_CFG, 0, True),
    "admin": Scenario(sc_admin, {}, 0, True),
}
# judged by the record alone, on the HIP plane: the golden model has neither a step's egress budget
# nor its delivery-slot bound nor a pair table
DEVICE_ONLY = {
    "budget_cut": Scenario(sc_budget_cut, BUDGET_CFG, 0, True),
    "slot_cut": Scenario(sc_slot_cut, SLOT_CFG, 0, True),
    "pair_cut": Scenario(sc_pair_cut, PAIR_CFG, 0, True),
}
WIDTHS = {"narrow": {}, "wide": TWO_PASS}
OFF = Scenario(sc_off, {}, 0, True)
