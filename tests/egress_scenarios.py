"""The back of the step -- the delivery layout (k_dv_write, the delivery-size scan of
k_conn_layout, k_post's tag hand-over), the connection layout (k_conn_layout and its twin
k_conn_sizes / k_scan / k_conn_out, set_egress_bytes and the gather table), the render
(k_render: render_return, render_confirms, render_deliv) and the persist pack (k_persist_size
/ k_persist_pack) -- at the places where those kernels change path, in the style of
``consumer_scenarios``, ``ingress_scenarios`` and ``route_scenarios``.

A scenario is ``(dp, lim, env) -> Run``.  It declares its topology and sends its traffic
through a ``Net``, which applies both to the plane and keeps its own record of them: queues
as lists, channels with their tags, windows and confirm counts, consumers with their credit.
From that record alone ``Net.step`` renders what every connection must receive in the step,
with the host codec (``render_command`` at the connection's frame-max, pinned against the
reference by test_codec.py; ``command`` is that function with the header frame kept between
calls), in the region order the kernels document:

1. returns, in publish order;
2. one confirm frame per confirm-mode channel with publishes, in channel-slot order;
3. deliveries in channel-slot order then run order (queue slot, Basic.Get answers ahead of
   the queue's consumers, consumers from the queue's round-robin start), a Basic.GetOk where
   the run is a Get;
4. the connection's Basic.GetEmpty frames.

The record never calls the golden model or ``models/matcher.py``: routing is a dict for the
default and direct exchanges and a list for fanout.  The dispatch rule it follows is the one
the data plane documents (QueueEntity's round robin as the step splits it): a queue's ready
messages go to its consumers from the round-robin start, ``ceil(remaining / consumers left)``
each, cut by the consumer's prefetch credit, the channel's window and ``deliver_cap``; the
start moves by one for every step in which the queue dispatched.

``check_run`` judges a run: ``egress[conn] == expected[conn]`` for every connection and
step; and, walking the frames the plane sent on their own, no frame larger than its
connection's frame-max, delivery tags counting up from the channel's previous tag, confirm
tags continuing from the previous step by the number of publishes the scenario sent.  The
counters a scenario names (``n_deliv``, ``n_returns``, the run count, ``n_ref`` ..) are
compared where the plane keeps them.

Every scenario that depends on a count or a placement asserts it while it is built, and
``Run.placed`` records what was asserted.  ``lim`` holds the kernels' limits as the built
extension exports them (``limits()``).
"""

import random
import struct
from collections import defaultdict, namedtuple

from chanamq_amd.engine.traffic import ack_frame
from chanamq_amd.protocol.codec import (Method, decode_method, encode_content_header, encode_frame, encode_method_frame,
                                        encode_properties, render_command)
from dp_scenarios import NOW, VH

Scenario = namedtuple("Scenario", "fn cfg")
Run = namedtuple("Run", "steps net placed")
Limits = namedtuple("Limits", "DVW_LDS CONN_LAYOUT_MAX RC_RET_BLOCKS RD_G")
Env = namedtuple("Env", "c_max chpc ucap deliver_cap ref_min")
Stat = namedtuple("Stat", "n_deliv n_runs n_returns n_confirm_frames n_ref ref_bytes n_live_msgs rendered")

DELIV_PASS = 16384    # deliveries one pass of k_conn_layout's size scan walks: 1024 threads x 16 entries
CONN_PASS = 1024      # connections one pass of its connection scan walks: one per thread
NO_ROUTE = "The exchange cannot route the result of a Publish"                           # 312
NO_CONSUMER = "The exchange cannot deliver to a consumer when the immediate flag is set"  # 313
REPLY = {312: NO_ROUTE, 313: NO_CONSUMER}
NO_PROPS = {}


def limits():
    """The delivery-layout and render limits, from the built extension."""
    from chanamq_amd import ops
    m = ops.load()
    return Limits(*(int(getattr(m, k)) for k in Limits._fields))


def env_of(dp, cfg):
    """What the record needs to know of the plane: table sizes, and the smallest referenced
    body (None: egress by reference is off)."""
    if hasattr(dp, "info"):
        i = dp.info
        ref = i["egress_ref_min"] if i["egress_ref_back"] >= 0 else None
        return Env(i["c_max"], i["chpc"], i["ucap"], i["deliver_cap"], ref)
    ref = None if cfg.get("egress_ref", 0) is None else max(cfg.get("egress_ref_min", 256), 16)
    return Env(dp.c_max, dp.chpc, dp.ucap, dp.deliver_cap, ref)


def is_golden(dp):
    return not hasattr(dp, "eng")


NOISE = random.Random(20).randbytes(1 << 16)


def body_of(i, size):
    """The body of the run's i-th publish: a window of fixed noise that starts elsewhere for
    every publish, so a shifted or a misplaced byte shows."""
    at = (7919 * i) % (len(NOISE) - size)
    return NOISE[at:at + size]


_frames = {}


def command(num, method, props=None, body=b"", fm=131072):
    """``render_command`` with the content header's frame kept for the next command of the
    same channel, size and properties (a step of 16 384 deliveries renders as many): the
    method frame, the header and the body frames split at ``fm`` - 8 as the codec makes them."""
    if not method.has_content:
        return encode_method_frame(num, method)
    key = (num, len(body), id(props))
    hit = _frames.get(key)
    if hit is None or hit[0] is not props:
        hit = _frames[key] = (props, encode_frame(2, num, encode_content_header(method.class_id, len(body), props or {})))
    parts = [encode_method_frame(num, method), hit[1]]
    for i in range(0, len(body), fm - 8):
        parts.append(encode_frame(3, num, body[i:i + fm - 8]))
    return b"".join(parts)


# ---------------------------------------------------------------- the record
class Chan:
    def __init__(self, conn, num, local, chslot):
        self.conn, self.num, self.local, self.chslot = conn, num, local, chslot
        self.confirm, self.prefetch = False, 0
        self.next_tag, self.uhead, self.reserved, self.confirm_next = 1, 1, 0, 1
        self.slots = {}           # delivery tag -> [done, message, consumer, queue]

    def win(self):
        return self.next_tag - self.uhead + self.reserved


class Cons:
    def __init__(self, chan, queue, tag, no_ack):
        self.chan, self.queue, self.tag, self.no_ack, self.unacked = chan, queue, tag, no_ack, 0


class Queue:
    def __init__(self, name, slot, durable, bound):
        self.name, self.slot, self.durable, self.bound = name, slot, durable, bound
        self.ready, self.consumers, self.rr, self.tail, self.back = [], [], 0, 0, []


class Msg:
    def __init__(self, serial, step, ex, rk, props, body, persistent, one_frame):
        self.serial, self.step, self.ex, self.rk, self.props, self.body = serial, step, ex, rk, props, body
        self.persistent, self.one_frame, self.refs = persistent, one_frame, 0


class Net:
    """The scenario's own record of the topology and the traffic, and of what every
    connection must receive."""

    def __init__(self, dp, env):
        self.dp, self.env = dp, env
        self.frame_max, self.chans, self.queues = {}, {}, {}
        self.xtype, self.binds = {"": "direct"}, defaultdict(list)
        self.cur, self.events = defaultdict(list), defaultdict(list)       # per connection: wire chunks, events
        self.nxt, self.nxt_events = defaultdict(list), defaultdict(list)
        self.steps, self.expected, self.stats, self.persist, self.pubcount = [], [], [], [], []
        self.serial, self.frags, self._live = 0, [], []

    # ---- topology
    def conn(self, conn, frame_max=None):
        if conn in self.frame_max:
            return
        if frame_max is None:
            self.dp.open_connection(conn, VH)
        else:
            self.dp.open_connection(conn, VH, frame_max=frame_max)
        self.frame_max[conn] = frame_max or 131072

    def chan(self, conn, num, confirm=False, prefetch=0):
        self.conn(conn)
        if (conn, num) in self.chans:
            return self.chans[(conn, num)]
        local = sum(1 for c, _ in self.chans if c == conn)       # channel slots in opening order
        self.dp.open_channel(conn, num)
        ch = self.chans[(conn, num)] = Chan(conn, num, local, conn * self.env.chpc + local)
        assert self.dp.chslot(conn, num) == ch.chslot and local < self.env.chpc
        if confirm:
            self.dp.confirm_select(conn, num)
            ch.confirm = True
        if prefetch:
            self.dp.qos(conn, num, prefetch_count=prefetch)
            ch.prefetch = prefetch
        return ch

    def queue(self, name, durable=False, capacity=None, bounded=False):
        """``bounded``: a ring of ``capacity`` that cannot grow (a publish to a full one is
        dropped and its channel's confirm of the step is a Basic.Nack)."""
        kw = dict(durable=durable)
        if capacity:
            kw.update(capacity=capacity, max_capacity=capacity if bounded else 0)
        slot = self.dp.declare_queue(VH, name, **kw)
        assert all(q.slot != slot for q in self.queues.values())
        self.queues[name] = Queue(name, slot, durable, capacity if bounded else None)
        self.binds[""].append((name, name))
        return slot

    def exchange(self, name, type_):
        assert type_ in ("direct", "fanout")
        self.dp.declare_exchange(VH, name, type_)
        self.xtype[name] = type_

    def bind(self, q, x, key):
        self.dp.bind(VH, q, x, key)
        self.binds[x].append((q, key))

    def consume(self, conn, num, q, tag, no_ack=True):
        ch = self.chans[(conn, num)]
        self.dp.consume(conn, num, VH, q, tag, no_ack=no_ack)
        self.queues[q].consumers.append(Cons(ch, self.queues[q], tag, no_ack))

    def route(self, x, key):
        if x not in self.xtype:
            return None
        hit = {q for q, k in self.binds[x] if self.xtype[x] == "fanout" or k == key}
        return sorted((self.queues[q] for q in hit), key=lambda q: q.slot)

    # ---- traffic of the step under construction
    def pub(self, conn, num, x, key, body, props=None, mandatory=False, immediate=False, piece=None, hold=0):
        """One publish on the wire, its body in frames of ``piece`` bytes (the connection's
        frame-max less 8 by default).  ``hold``: its last ``hold`` bytes arrive with the next
        step, which is then the step the publish belongs to."""
        fm = self.frame_max[conn]
        piece = piece or fm - 8
        assert 0 < piece <= fm - 8
        props = props or NO_PROPS
        m = Method("basic.publish", exchange=x, routing_key=key, mandatory=mandatory, immediate=immediate)
        data = command(num, m, props, body, piece + 8)
        nfr = -(-len(body) // piece)
        self.frags.append(nfr)
        ev = ("pub", num, x, key, body, props, mandatory, immediate, nfr == 1 and not hold)
        if hold:
            assert 0 < hold < len(data) and not self.nxt[conn]
            self.cur[conn].append(data[:-hold])
            self.nxt[conn].append(data[-hold:])
            self.nxt_events[conn].append(ev)
        else:
            self.cur[conn].append(data)
            self.events[conn].append(ev)

    def ack(self, conn, num, tag, multiple=False):
        self.cur[conn].append(ack_frame(num, tag, multiple=multiple))
        self.events[conn].append(("ack", num, tag, multiple, False))

    def nack_requeue(self, conn, num, tag):
        self.cur[conn].append(render_command(num, Method("basic.nack", delivery_tag=tag, multiple=False, requeue=True)))
        self.events[conn].append(("ack", num, tag, False, True))

    def get(self, conn, num, q, no_ack=True):
        """Basic.Get, served by the step itself.  Only the same Get may follow it in the
        connection's bytes of the step: send it last."""
        self.cur[conn].append(render_command(num, Method("basic.get", ticket=0, queue=q, no_ack=no_ack)))
        self.events[conn].append(("get", num, q, no_ack))

    def outstanding(self, conn, num):
        return any(not s[0] for s in self.chans[(conn, num)].slots.values())

    # ---- one step: what it must lead to
    def step(self, ops=None):
        k = len(self.steps)
        inp = {c: b"".join(d) for c, d in self.cur.items() if d}
        if ops:
            inp["__ops__"] = list(ops)
        self.steps.append(inp)
        returns, pub_cnt, fail = defaultdict(list), defaultdict(int), set()
        settles, gets, precs = [], defaultdict(list), []
        for conn in sorted(self.events):
            seen_get = False
            for ev in self.events[conn]:
                assert not seen_get or ev[0] == "get", "a Basic.Get is the last thing a connection sends in a step"
                if ev[0] == "pub":
                    self._publish(k, conn, ev, returns, pub_cnt, fail, precs)
                elif ev[0] == "ack":
                    settles.append((self.chans[(conn, ev[1])],) + ev[2:])
                else:
                    seen_get = True
                    gets[ev[2]].append((self.chans[(conn, ev[1])], ev[3]))
        for ch, tag, multiple, requeue in settles:
            self._settle(ch, tag, multiple, requeue)
        for q in self.queues.values():          # requeued messages go back in front, oldest first
            if q.back:
                q.ready[:0] = [(m, True) for m in sorted(q.back, key=lambda m: m.serial)]
                q.back = []
        for ch in self.chans.values():          # the window's head moves over what is settled
            while ch.uhead in ch.slots and ch.slots[ch.uhead][0]:
                del ch.slots[ch.uhead]
                ch.uhead += 1
        delivs, gempty, runs = [], defaultdict(list), 0
        for q in sorted(self.queues.values(), key=lambda q: q.slot):
            runs += self._dequeue(q, gets.get(q.name, ()), delivs, gempty)
        delivs.sort(key=lambda d: d["chan"].chslot)   # (stable: run order within a channel)
        n_ref = ref_bytes = 0
        by_conn = defaultdict(list)
        for d in delivs:
            ch = d["chan"]
            d["tag"] = ch.next_tag
            ch.next_tag += 1
            ch.reserved -= 1
            ch.slots[d["tag"]] = [d["noack"], d["msg"], d["cons"], d["queue"]]
            if d["noack"]:
                d["msg"].refs -= 1
            m, fm = d["msg"], self.frame_max[ch.conn]
            if (self.env.ref_min is not None and m.step == k and m.one_frame and len(m.body) >= self.env.ref_min
                    and len(m.body) <= fm - 8):
                n_ref += 1
                ref_bytes += len(m.body)
            by_conn[ch.conn].append(d)
        out, nconf = {}, 0
        for conn in sorted(self.frame_max):
            parts = list(returns.get(conn, ()))
            for ch in sorted((c for c in self.chans.values() if c.conn == conn), key=lambda c: c.local):
                n = pub_cnt.get(ch.chslot, 0)
                if not n or not ch.confirm:
                    continue
                last = ch.confirm_next + n - 1
                ch.confirm_next = last + 1
                if ch.chslot in fail:
                    m = Method("basic.nack", delivery_tag=last, multiple=n > 1, requeue=False)
                else:
                    m = Method("basic.ack", delivery_tag=last, multiple=n > 1)
                parts.append(render_command(ch.num, m))
                nconf += 1
            for d in by_conn.get(conn, ()):
                parts.append(self._deliver(d, self.frame_max[conn]))
            for num in gempty.get(conn, ()):
                parts.append(render_command(num, Method("basic.get_empty", cluster_id="")))
            if parts:
                out[conn] = b"".join(parts)
        self.expected.append(out)
        self.persist.append(precs)
        self.pubcount.append({(c.conn, c.num): pub_cnt[c.chslot] for c in self.chans.values() if pub_cnt.get(c.chslot)})
        live = sum(1 for m in self._live if m.refs > 0)
        self._live = [m for m in self._live if m.refs > 0]
        st = Stat(len(delivs), runs, sum(map(len, returns.values())), nconf, n_ref, ref_bytes, live,
                  sum(map(len, out.values())) - ref_bytes)
        self.stats.append(st)
        self.cur, self.events = self.nxt, self.nxt_events
        self.nxt, self.nxt_events = defaultdict(list), defaultdict(list)
        return st

    def _publish(self, k, conn, ev, returns, pub_cnt, fail, precs):
        _, num, x, key, body, props, mandatory, immediate, one_frame = ev
        ch = self.chans[(conn, num)]
        if ch.confirm:
            pub_cnt[ch.chslot] += 1
        qs = self.route(x, key)
        assert qs is not None, "publishes to unknown exchanges are another scenario module's"
        code = 0
        if not qs:
            code = 312 if mandatory else 0
        elif immediate and not any(q.consumers for q in qs):
            code, qs = 313, []
        if code:
            m = Method("basic.return", reply_code=code, reply_text=REPLY[code], exchange=x, routing_key=key)
            returns[conn].append(command(num, m, props, body, self.frame_max[conn]))
        if not qs:
            return
        msg = Msg(self.serial, k, x, key, props, body, props.get("delivery_mode") == 2, one_frame)
        self.serial += 1
        self._live.append(msg)
        for q in qs:
            if q.bound is not None and len(q.ready) >= q.bound:
                fail.add(ch.chslot)
                continue
            msg.refs += 1
            if q.durable and msg.persistent:
                precs.append((q.slot, q.tail, x.encode(), key.encode(), encode_properties(props), body, msg.serial))
            q.tail += 1
            q.ready.append((msg, False))

    def _settle(self, ch, tag, multiple, requeue):
        tags = [t for t in sorted(ch.slots) if not ch.slots[t][0] and (t <= tag or tag == 0)] if multiple else \
               [t for t in (tag,) if t in ch.slots and not ch.slots[t][0]]
        for t in tags:
            s = ch.slots[t]
            s[0] = True
            if s[2] is not None:
                s[2].unacked -= 1
            if requeue:
                s[3].back.append(s[1])
            else:
                s[1].refs -= 1

    def _dequeue(self, q, gets, delivs, gempty):
        runs = ngot = 0
        for ch, no_ack in gets:
            if not q.ready:
                gempty[ch.conn].append(ch.num)
                continue
            assert ngot < 32 and ch.win() < self.env.ucap, "a Get the step would hand to the host"
            msg, red = q.ready.pop(0)
            ch.reserved += 1
            delivs.append(dict(chan=ch, cons=None, queue=q, msg=msg, red=red, noack=no_ack, left=len(q.ready)))
            ngot += 1
            runs += 1
        m = len(q.consumers)
        if not m or not q.ready:
            return runs
        assert m + ngot <= 64, "more consumers than a step's runs of one queue"
        r, remaining = q.rr % m, len(q.ready)
        for j in range(m):
            c = q.consumers[(r + j) % m]
            g = 0
            if remaining:
                want = min(-(-remaining // (m - j)), self.env.deliver_cap)
                if not c.no_ack and c.chan.prefetch:
                    want = min(want, max(c.chan.prefetch - c.unacked, 0))
                g = min(want, self.env.ucap - c.chan.win())
            for _ in range(g):
                msg, red = q.ready.pop(0)
                delivs.append(dict(chan=c.chan, cons=c, queue=q, msg=msg, red=red, noack=c.no_ack))
            c.chan.reserved += g
            if not c.no_ack:
                c.unacked += g
            remaining -= g
            runs += 1 if g else 0
        q.rr = (r + 1) % m
        return runs

    @staticmethod
    def _deliver(d, fm):
        msg = d["msg"]
        if d["cons"] is None:
            m = Method("basic.get_ok", delivery_tag=d["tag"], redelivered=d["red"], exchange=msg.ex, routing_key=msg.rk,
                       message_count=d["left"])
        else:
            m = Method("basic.deliver", consumer_tag=d["cons"].tag, delivery_tag=d["tag"], redelivered=d["red"],
                       exchange=msg.ex, routing_key=msg.rk)
        return command(d["chan"].num, m, msg.props, msg.body, fm)

    def run(self, **placed):
        assert not any(self.cur.values()) and not any(self.nxt.values()) and placed
        return Run(self.steps, self, placed)


# ---------------------------------------------------------------- runner
COUNTERS = ("n_deliv", "n_returns", "n_confirm_frames", "n_ref", "ref_bytes", "n_live_msgs", "live_bytes", "n_ring_full",
            "n_unroutable", "n_persist", "persist_used")
SHARED = ("n_deliv", "n_ring_full", "n_unroutable")   # the golden model counts these too


def run_egress(dp, steps, persist=False):
    """Drive dp through the steps (control ops first): the outputs of ``dp_scenarios.run``
    plus the step's counters, on the HIP plane its run count (``n_runs``), and with
    ``persist`` the step's persist records."""
    outs = []
    for k, inp in enumerate(steps):
        inp = dict(inp)
        for op in inp.pop("__ops__", []):
            getattr(dp, op[0])(*op[1], **(op[2] if len(op) > 2 else {}))
        r = dp.step(inp, now_ms=NOW)
        if isinstance(r, dict):
            eg, ctrl, ev, segs, tx, cnt = r["egress"], r["ctrl"], r["events"], r["segs"], r.get("txbuf", []), r["counters"]
        else:
            eg, ctrl, ev, segs, tx, cnt = r.egress, r.ctrl, r.events, [s[:4] for s in r.segs], r.txbuf, r.counters
        o = dict(egress=eg, ctrl=sorted(ctrl), events=sorted(ev), gets=[], txbuf=sorted(tx),
                 segs=sorted((s[0], s[1], s[2], s[3]) for s in segs),
                 counters={c: int(cnt[c]) for c in COUNTERS if c in cnt})
        if not is_golden(dp):
            o["counters"]["n_runs"] = int(dp.eng.step_runs(dp._last_parity))
        if persist:
            if not is_golden(dp):
                o["persist_raw"] = dp.take_persist_raw()[0]
            o["persist"] = dp.take_persist()
        outs.append(o)
    return outs


def golden_plane(cfg):
    """The golden model with the engine config ``cfg`` (gpu_cfg.CFG + a scenario's overrides)."""
    from chanamq_amd.engine.golden import GoldenDataPlane
    from consumer_scenarios import GOLDEN_KEYS
    kw = {k: cfg[k] for k in GOLDEN_KEYS + ("ring_pool", "deliv_max", "egress_cap") if k in cfg}
    return GoldenDataPlane(persist=bool(cfg.get("persist")), **kw)


# ---------------------------------------------------------------- the checks
def first_diff(a, b):
    n = min(len(a), len(b))
    return next((i for i in range(n) if a[i] != b[i]), n)


def check_bytes(run, outs):
    """egress[conn] == expected[conn], every connection, every step."""
    assert len(outs) == len(run.net.expected)
    for k, (o, want) in enumerate(zip(outs, run.net.expected)):
        got = {c: bytes(d) for c, d in o["egress"].items() if len(d)}
        assert sorted(got) == sorted(want), f"step {k}: egress for connections {sorted(got)}, expected {sorted(want)}"
        for c in sorted(want):
            if got[c] != want[c]:
                at = first_diff(got[c], want[c])
                raise AssertionError(f"step {k} conn {c}: {len(got[c])} bytes, expected {len(want[c])}; first difference at "
                                     f"byte {at}: {got[c][at:at + 16].hex()} for {want[c][at:at + 16].hex()}")


def check_wire(run, outs):
    """The frames as sent, walked on their own: none larger than the connection's frame-max,
    every frame well formed; delivery tags count up from the channel's previous tag; confirm
    tags continue from the previous step by the publishes the scenario sent."""
    net = run.net
    dtag, ctag = defaultdict(int), defaultdict(int)
    for k, o in enumerate(outs):
        confirmed = set()
        for conn in sorted(o["egress"]):
            data, pos, fm = bytes(o["egress"][conn]), 0, net.frame_max[conn]
            while pos < len(data):
                assert pos + 8 <= len(data), f"step {k} conn {conn}: egress ends inside a frame header"
                t, ch, size = struct.unpack_from(">BHI", data, pos)
                end = pos + 8 + size
                assert t in (1, 2, 3) and end <= len(data) and data[end - 1] == 0xCE, f"step {k} conn {conn}: bad frame at {pos}"
                assert 8 + size <= fm, f"step {k} conn {conn}: a frame of {8 + size} bytes, frame-max {fm}"
                if t == 1:
                    m = decode_method(data[pos + 7:end - 1])
                    if m.name in ("basic.deliver", "basic.get_ok"):
                        dtag[(conn, ch)] += 1
                        assert m.delivery_tag == dtag[(conn, ch)], (
                            f"step {k} channel {(conn, ch)}: delivery tag {m.delivery_tag}, expected {dtag[(conn, ch)]}")
                    elif m.name in ("basic.ack", "basic.nack"):
                        n = net.pubcount[k].get((conn, ch), 0)
                        assert n and (conn, ch) not in confirmed, f"step {k} channel {(conn, ch)}: a confirm for nothing"
                        confirmed.add((conn, ch))
                        ctag[(conn, ch)] += n
                        assert m.delivery_tag == ctag[(conn, ch)] and bool(m.multiple) == (n > 1), (
                            f"step {k} channel {(conn, ch)}: confirm up to {m.delivery_tag}, multiple {m.multiple}; "
                            f"expected {ctag[(conn, ch)]} after {n} publishes")
                pos = end
        want = {c for c, n in net.pubcount[k].items() if n and net.chans[c].confirm}
        assert confirmed == want, f"step {k}: confirms on {sorted(confirmed)}, expected {sorted(want)}"


GPU_ONLY = ("n_runs", "n_returns", "n_confirm_frames", "n_ref", "ref_bytes", "n_live_msgs")


def check_counters(run, outs, golden):
    for k, (o, st) in enumerate(zip(outs, run.net.stats)):
        c = o["counters"]
        assert c["n_deliv"] == st.n_deliv, f"step {k}: n_deliv {c['n_deliv']}, expected {st.n_deliv}"
        if golden:
            continue
        for f in GPU_ONLY:
            assert c[f] == getattr(st, f), f"step {k}: {f} {c[f]}, expected {getattr(st, f)}"


def check_run(run, outs, golden=False):
    check_bytes(run, outs)
    check_wire(run, outs)
    check_counters(run, outs, golden)


def check_drained(outs):
    c = outs[-1]["counters"]
    assert c["n_live_msgs"] == 0 and c["live_bytes"] == 0, f"{c['n_live_msgs']} messages, {c['live_bytes']} bytes still live"


# ================================================================ delivery layout
RUN_QUEUES, RUN_CONS = 57, 9


def sc_runs_lds(dp, lim, env):
    """57 queues with 9 manual-ack consumers each.  Consumer i of queues 3g, 3g + 1 and 3g + 2
    share channel 9g + i, so a channel's deliveries of a step span three runs and the
    ``last``-of-channel test looks across runs.  The channels of queues 0..2 have prefetch 2,
    the others prefetch 1.  A step publishes 9 messages to a queue (18 to queue 0: its nine
    runs have ``cnt`` 2) and fewer to the last one, so that exactly DVW_LDS - 1, DVW_LDS and
    DVW_LDS + 1 consumers are granted: k_dv_write stages the runs in LDS in the first two steps
    and searches global memory in the third.  Every consumer acks everything before the next
    step's publishes, and the round-robin start moves, so the runs change channels."""
    net = Net(dp, env)
    net.chan(1, 1)
    for q in range(RUN_QUEUES):
        net.queue(f"r{q:02d}")
    chans = []
    for q in range(RUN_QUEUES):
        for i in range(RUN_CONS):
            ci = (q // 3) * RUN_CONS + i
            conn, num = 2 + ci // env.chpc, 1 + ci % env.chpc
            if (conn, num) not in net.chans:
                net.chan(conn, num, prefetch=2 if q < 3 else 1)
                chans.append((conn, num))
            net.consume(conn, num, f"r{q:02d}", f"c{q:02d}.{i}", no_ack=False)
    per_chan = defaultdict(set)
    for q in net.queues.values():
        for c in q.consumers:
            per_chan[c.chan.chslot].add(q.name)
    assert all(len(v) == 3 for v in per_chan.values()) and len(per_chan) == 19 * RUN_CONS
    counts = [lim.DVW_LDS - 1, lim.DVW_LDS, lim.DVW_LDS + 1]
    assert counts[-1] <= RUN_QUEUES * RUN_CONS and counts[0] > RUN_CONS
    serial = 0
    for n in counts:
        for conn, num in chans:
            if net.outstanding(conn, num):
                net.ack(conn, num, 0, multiple=True)
        full, rest = divmod(n, RUN_CONS)
        for q in range(full + (1 if rest else 0)):
            for _ in range((2 * RUN_CONS if q == 0 else RUN_CONS) if q < full else rest):
                net.pub(1, 1, "", f"r{q:02d}", body_of(serial, 5 + serial % 7))
                serial += 1
        st = net.step()
        assert st.n_runs == n and st.n_deliv == n + RUN_CONS, st
    for conn, num in chans:
        net.ack(conn, num, 0, multiple=True)
    assert net.step().n_deliv == 0
    assert net.step().n_live_msgs == 0
    return net.run(runs=counts, channels=len(chans))


DELIV_COUNTS = (DELIV_PASS - 1, DELIV_PASS, DELIV_PASS + 1, DELIV_PASS + 16)
DELIV_CONNS = 5
DELIV_PUBLISHERS = 10     # (a connection's bytes of one step stay below the frame scan's candidate limit)


def sc_deliv_passes(dp, lim, env):
    """Five auto-ack consumers on five connections and bodies of 8 bytes: four steps deliver
    16 383, 16 384, 16 385 and 16 400 messages -- one pass of the delivery-size scan less one
    entry (the last thread's 16 entries take the scalar path), exactly one pass, one entry
    into a second pass and one whole vector of 16 into it.  The last connection's deliveries
    straddle the pass boundary in the last two steps, so its region's size is a difference of
    offsets from two passes."""
    net = Net(dp, env)
    for p in range(DELIV_PUBLISHERS):
        net.chan(20 + p, 1)
    for i in range(DELIV_CONNS):
        net.queue(f"d{i}", capacity=4096)
        net.chan(10 + i, 1)
        net.consume(10 + i, 1, f"d{i}", f"c{i}")
    serial, spans = 0, []
    for n in DELIV_COUNTS:
        per = [n // DELIV_CONNS + (1 if i < n % DELIV_CONNS else 0) for i in range(DELIV_CONNS)]
        for i, cnt in enumerate(per):
            for _ in range(cnt):
                net.pub(20 + serial % DELIV_PUBLISHERS, 1, "", f"d{i}", body_of(serial, 8))
                serial += 1
        st = net.step()
        assert st.n_deliv == n and st.n_runs == DELIV_CONNS and max(per) <= min(env.ucap, env.deliver_cap)
        spans.append((n - per[-1], n))
    assert [n % 16 for n in DELIV_COUNTS] == [15, 0, 1, 0]
    assert all(lo < DELIV_PASS < hi for lo, hi in spans[2:]) and all(hi <= DELIV_PASS for _, hi in spans[:2])
    assert net.step().n_live_msgs == 0
    return net.run(n_deliv=list(DELIV_COUNTS), last_conn=spans)


def sc_mixed_channel(dp, lim, env):
    """Channel A holds an auto-ack consumer of one queue, a manual-ack consumer of another and
    a Basic.Get answer, all in one step: its window head cannot move over the pending
    manual-ack slots, so it is left to the window walk.  Channel B is pure auto-ack: its head
    moves in k_dv_write itself, and over four steps it takes more messages than the window
    has slots.  Then channel A takes manual-ack deliveries again, a second Get empties the Get
    queue (message-count 0), and after the last ack nothing lives."""
    net = Net(dp, env)
    net.chan(1, 1)
    for q in ("m1", "m2", "mg", "mb"):
        net.queue(q)
    a, b = (2, 5), (2, 6)
    net.chan(*a)
    net.chan(*b)
    net.consume(*a, "m1", "auto", no_ack=True)
    net.consume(*a, "m2", "manual", no_ack=False)
    net.consume(*b, "mb", "bulk", no_ack=True)
    serial = [0]

    def pubs(q, n):
        for _ in range(n):
            net.pub(1, 1, "", q, body_of(serial[0], 10 + serial[0] % 23))
            serial[0] += 1
    per = env.ucap // 2 - 20
    pubs("m1", 3), pubs("m2", 2), pubs("mg", 2), pubs("mb", per)
    net.get(*a, "mg", no_ack=False)
    st = net.step()
    kinds = {(d[2] is None, d[0]) for d in net.chans[a].slots.values()}
    assert st.n_deliv == 6 + per and kinds == {(False, True), (False, False), (True, False)}
    assert net.chans[a].uhead < net.chans[a].next_tag and net.chans[b].win() == per
    total = per
    for _ in range(3):
        pubs("mb", per)
        total += per
        assert net.step().n_deliv == per
    assert total > env.ucap
    pubs("m1", 2), pubs("m2", 3)
    net.get(*a, "mg", no_ack=True)
    st = net.step()
    assert st.n_deliv == 6 and st.n_live_msgs == 6          # 5 manual-ack deliveries and the Get's
    net.ack(*a, 0, multiple=True)
    net.step()
    assert net.step().n_live_msgs == 0
    return net.run(bulk=total, per_step=per)


# ================================================================ connection layout
CH_NUMS = (700, 3, 65535, 9, 1, 40000, 2, 12)     # channel numbers in opening order: out of slot order on the wire
PUBLISHER = 5


def regions_open(net, conn, k):
    """One connection that will carry all four regions, copy ``k`` (its queues carry k in
    their names).  It opens as many channels as the plane has per connection; slots 0, 2 and 4
    are in confirm mode."""
    n = net.env.chpc
    nums = CH_NUMS[:n]
    for i, num in enumerate(nums):
        net.chan(conn, num, confirm=i in (0, 2, 4))
    role = lambda i: nums[i % n]
    net.queue(f"qi{k}")
    net.queue(f"qr{k}")
    net.queue(f"qg{k}")
    net.queue(f"full{k}", capacity=4, bounded=True)
    net.queue(f"lone{k}")
    net.consume(conn, role(1), f"qi{k}", f"inline-{k}", no_ack=True)
    net.consume(conn, role(3), f"qr{k}", f"byref-{k}", no_ack=False)
    return role


def regions_prefill(net, k, serial):
    for _ in range(4):
        net.pub(PUBLISHER, 1, "", f"full{k}", body_of(serial + k, 3))
    net.pub(PUBLISHER, 1, "", f"qg{k}", body_of(serial + 7 + k, 30))


def regions_traffic(net, conn, k, role, serial):
    """All four regions in one step: a 312 and a 313 return; a Basic.Ack with multiple 0, one
    with multiple 1 and a Basic.Nack (confirm channels with 1, 3 and 2 publishes, the last
    into a full ring) where the plane has the channels for it; inline and referenced
    deliveries and a GetOk; two GetEmpty."""
    rm = net.env.ref_min or 256
    net.pub(conn, role(0), "", f"qi{k}", body_of(serial, 20))
    net.pub(conn, role(2), "", f"qi{k}", body_of(serial + 1, 40), props={"content_type": "a/b"})
    net.pub(conn, role(2), "", f"qr{k}", body_of(serial + 2, rm + 44))
    net.pub(conn, role(2), "dx", f"qr{k}", body_of(serial + 3, rm))
    net.pub(conn, role(4), "", f"full{k}", body_of(serial + 4, 9))
    net.pub(conn, role(4), "", f"full{k}", body_of(serial + 5, 9))
    net.pub(conn, role(7), "dx", "nobody", body_of(serial + 6, 33), mandatory=True)
    net.pub(conn, role(7), "", f"lone{k}", body_of(serial + 7, 0), immediate=True)
    net.pub(conn, role(7), "", f"qi{k}", body_of(serial + 8, rm - 1))
    for _ in range(3):
        net.get(conn, role(6), f"qg{k}", no_ack=True)


def regions_run(dp, env, mains, conf_only, gempty_only, silent, placed):
    """The four-region traffic on every connection slot of ``mains``, with a connection that
    has confirms only, one with GetEmpty only and an open one with nothing."""
    net = Net(dp, env)
    net.chan(PUBLISHER, 1)
    net.exchange("dx", "direct")
    roles = {c: regions_open(net, c, k) for k, c in enumerate(mains)}
    for k in range(len(mains)):
        net.bind(f"qr{k}", "dx", f"qr{k}")
    net.queue("sink")
    net.queue("void")
    net.chan(conf_only, 8, confirm=True)
    net.chan(gempty_only, 4)
    if silent is not None:
        net.chan(silent, 1)
    for k in range(len(mains)):
        regions_prefill(net, k, 100 * k)
    assert net.step().n_deliv == 0
    for k, c in enumerate(mains):
        regions_traffic(net, c, k, roles[c], 1000 + 100 * k)
    net.pub(conf_only, 8, "", "sink", body_of(77, 12))
    net.pub(conf_only, 8, "", "sink", body_of(78, 12))
    net.get(gempty_only, 4, "void")
    st = net.step()
    out = net.expected[-1]
    assert sorted(out) == sorted(list(mains) + [conf_only, gempty_only])
    assert st.n_returns == 2 * len(mains) and st.n_deliv == 6 * len(mains) and st.n_runs == 3 * len(mains)
    assert st.n_ref == (2 * len(mains) if env.ref_min is not None else 0)
    for k, c in enumerate(mains):        # every region is there, in the documented order
        names = [decode_method(f[7:-1]).name for f in frames_of(out[c]) if f[0] == 1]
        order = [n for i, n in enumerate(names) if i == 0 or names[i - 1] != n]
        conf = [n for n in order if n in ("basic.ack", "basic.nack")]
        assert [n for n in order if n not in ("basic.ack", "basic.nack")] == \
            ["basic.return", "basic.deliver", "basic.get_ok", "basic.get_empty"] or env.chpc < 8, order
        assert names.count("basic.return") == 2 and names.count("basic.get_empty") == 2 and conf
        if env.chpc >= 8:
            assert [n for n in names if n in ("basic.ack", "basic.nack")] == ["basic.ack", "basic.ack", "basic.nack"]
            chs = [struct.unpack_from(">H", f, 1)[0] for f in frames_of(out[c]) if f[0] == 1]
            assert chs != sorted(chs)    # channel-slot order is not channel-number order
    assert len(out[conf_only]) == 21 and len(out[gempty_only]) == 13
    for c in mains:
        net.ack(c, roles[c](3), 0, multiple=True)
    net.step()
    assert net.step().n_live_msgs == 4 * len(mains) + 2       # what no consumer takes: the full rings', the sink's
    return net.run(mains=list(mains), **placed)


def frames_of(data):
    out, pos = [], 0
    while pos < len(data):
        size = struct.unpack_from(">I", data, pos + 3)[0]
        out.append(data[pos:pos + 8 + size])
        pos += 8 + size
    return out


def sc_conn_regions(dp, lim, env, last):
    """One connection with all four regions between a connection with confirms only, one with
    GetEmpty only and one with nothing.  ``last``: a second four-region connection sits on
    slot c_max - 1, whose thread publishes the step's egress_bytes and gath_off; without it
    that slot is silent and the same thread publishes them from an empty region."""
    mains = (7, env.c_max - 1) if last else (7,)
    return regions_run(dp, env, mains, 8, 9, 10, dict(last_slot=env.c_max - 1, last_busy=last))


def sc_conn_passes(dp, lim, env):
    """c_max 2048: two passes of the connection scan.  The four-region traffic sits on the
    last slot of the first pass, the first of the second and on c_max - 1."""
    assert env.c_max == 2 * CONN_PASS
    mains = (CONN_PASS - 1, CONN_PASS, env.c_max - 1)
    return regions_run(dp, env, mains, CONN_PASS - 2, CONN_PASS + 1, 3, dict(pass_size=CONN_PASS))


def sc_conn_wide(dp, lim, env):
    """c_max CONN_LAYOUT_MAX + 2: the engine lays connections out with k_conn_sizes, the
    scan and k_conn_out.  The four-region traffic on slots 0, CONN_LAYOUT_MAX - 1,
    CONN_LAYOUT_MAX and c_max - 1."""
    assert env.c_max == lim.CONN_LAYOUT_MAX + 2 and env.chpc == 1
    mains = (0, lim.CONN_LAYOUT_MAX - 1, lim.CONN_LAYOUT_MAX, env.c_max - 1)
    return regions_run(dp, env, mains, lim.CONN_LAYOUT_MAX - 2, 6, 3, dict(c_max=env.c_max))


WIDE_BASE_MAINS = (0, 20, 21, 63)


def sc_conn_wide_base(dp, lim, env):
    """The traffic of ``conn_wide`` on the single-block path (c_max 64): connection copy k
    must get the same bytes on both."""
    assert env.c_max <= lim.CONN_LAYOUT_MAX and env.chpc == 1
    return regions_run(dp, env, WIDE_BASE_MAINS, 19, 6, 3, dict(c_max=env.c_max))


def same_copies(wide, ow, base, ob):
    """Copy k of the four-region connection gets the same bytes in both runs."""
    pairs = list(zip(wide.placed["mains"], base.placed["mains"]))
    assert len(pairs) == 4 and len(ow) == len(ob)
    for k, (a, b) in enumerate(zip(ow, ob)):
        for cw, cb in pairs:
            assert a["egress"].get(cw, b"") == b["egress"].get(cb, b""), f"step {k}: connection {cw} against {cb}"
    assert all(len(ow[1]["egress"][cw]) > 500 for cw, _ in pairs)


# ================================================================ render
RET_FM = 4096
LONG = 255            # the longest exchange name / routing key the control plane accepts: a shortstr
HEADERS = {"headers": {f"key-{i:02d}": "v" * 11 for i in range(8)}}


def sc_return_frags(dp, lim, env):
    """A publisher with frame-max 4096 whose every publish comes back: mandatory to an
    exchange without bindings (a 255-byte name, keys of 0 and 255 bytes), mandatory to the
    default exchange with a key no queue has, and immediate to a queue (255-byte name) without
    a consumer.  Bodies of 0, 1, fm - 8, fm - 7 and 3 (fm - 8) + 5 bytes, each sent once in
    frames of fm - 8 bytes and once in frames of 1000, which straddle the 4088-byte frames of
    the return.  The largest one arrives in two steps and is joined through the carry.
    Properties from none to a headers table of about 200 bytes."""
    fm = RET_FM
    net = Net(dp, env)
    xl, ql = "x" * LONG, "l" * LONG
    net.exchange(xl, "direct")
    net.queue(ql)
    net.conn(3, frame_max=fm)
    net.chan(3, 7)
    net.chan(3, 9, confirm=True)
    sizes = [0, 1, fm - 8, fm - 7, 3 * (fm - 8) + 5]
    props = [None, {"content_type": "text/plain", "delivery_mode": 1}, HEADERS,
             {"message_id": "m" * 40, "priority": 3, "headers": {"a": 1}}]
    assert 190 <= len(encode_properties(HEADERS)) <= 230
    kinds = [dict(x=xl, key="", mandatory=True), dict(x="", key=ql, immediate=True),
             dict(x=xl, key="k" * LONG, mandatory=True), dict(x="", key="nosuchqueue", mandatory=True)]
    i = 0
    for piece in (fm - 8, 1000):
        for size in sizes:
            last = piece == 1000 and size == sizes[-1]
            net.pub(3, 7 if i % 3 else 9, body=body_of(i, size), props=props[i % len(props)], piece=piece,
                    hold=5000 if last else 0, **kinds[i % len(kinds)])
            i += 1
    frags = list(net.frags)
    assert frags == [0, 1, 1, 2, 4, 0, 1, 5, 5, 13] and (fm - 8) % 1000, frags
    st = net.step()
    assert st.n_returns == 9
    net.pub(3, 7, body=body_of(i, 1), **kinds[0])       # behind the joined one, in publish order
    st = net.step()
    assert st.n_returns == 2 and len(net.expected[-1][3]) > 3 * (fm - 8)
    assert net.step().n_returns == 0
    codes = [decode_method(f[7:-1]).reply_code for o in net.expected for f in frames_of(o.get(3, b"")) if f[0] == 1
             and decode_method(f[7:-1]).name == "basic.return"]
    assert codes.count(313) == 3 and codes.count(312) == 8
    return net.run(fragments=frags, held=5000)


def sc_return_flood(dp, lim, env):
    """RC_RET_BLOCKS * 4 + 1 returns in one step from three connections: the return waves'
    grid stride takes a second turn for exactly one.  Returns arrive in publish order per
    connection."""
    n = lim.RC_RET_BLOCKS * 4 + 1
    net = Net(dp, env)
    for c in (1, 2, 3):
        net.chan(c, 1)
    per = [n // 3 + 17, n // 3 - 17, n - 2 * (n // 3)]
    i = 0
    for c, cnt in zip((1, 2, 3), per):
        for _ in range(cnt):
            net.pub(c, 1, "", "none", body_of(i, i % 4), mandatory=True)
            i += 1
    st = net.step()
    assert st.n_returns == n == 2049 and sum(per) == n
    assert net.step().n_returns == 0
    return net.run(returns=n, per_conn=per)


CONFIRM_COUNTS = ([0, 1, 5, 0, 2, 1, 0, 3], [1, 0, 0, 7, 1, 0, 2, 1], [2, 2, 0, 0, 0, 1, 1, 0], [0, 0, 1, 1, 0, 0, 9, 0])


def sc_confirm_channels(dp, lim, env):
    """Every channel of connection 2 is in confirm mode; over four steps each has none, one or
    many publishes.  Channel slot 2 publishes into a ring of 4 that cannot grow: its fifth
    publish is dropped and the step's confirm is a Basic.Nack over the whole range, as is its
    one publish of the last step.  Connection 3 has a confirm channel and a plain one with
    publishes.  Tags continue across the steps without publishes and restart for nothing."""
    assert env.chpc == 8
    net = Net(dp, env)
    net.queue("sink")
    net.queue("tiny", capacity=4, bounded=True)
    for num in range(1, 9):
        net.chan(2, num, confirm=True)
    net.chan(3, 1, confirm=True)
    net.chan(3, 2)
    i, frames = 0, []
    for k, counts in enumerate(CONFIRM_COUNTS):
        for local, cnt in enumerate(counts):
            for _ in range(cnt):
                net.pub(2, 1 + local, "", "tiny" if local == 2 else "sink", body_of(i, 6))
                i += 1
        for _ in range((1, 0, 2, 0)[k]):
            net.pub(3, 1, "", "sink", body_of(i, 6))
            i += 1
        net.pub(3, 2, "", "sink", body_of(i, 6))
        net.pub(3, 2, "", "sink", body_of(i + 1, 6))
        i += 2
        st = net.step()
        frames.append(st.n_confirm_frames)
        names = [decode_method(f[7:-1]).name for f in frames_of(net.expected[-1].get(2, b""))]
        assert names.count("basic.nack") == (1 if counts[2] else 0)
    assert frames == [6, 5, 5, 3], frames
    return net.run(confirm_frames=frames)


def sc_deliver_fields(dp, lim, env):
    """Consumer tags of 0, 1, RD_G - 1, RD_G, RD_G + 1 and 255 bytes; exchange names and
    routing keys of 0, RD_G, RD_G + 1 and 255 bytes; bodies of 0, 1, RD_G - 1, RD_G and RD_G +
    1 bytes; properties of 0 and of more than 200 bytes: the group copies of render_deliv at
    one lane short of a stride, one stride and one byte into the next.  One delivery comes
    back flagged redelivered; Basic.GetOk frames carry message-counts 2, 1 and 0."""
    g = lim.RD_G
    net = Net(dp, env)
    net.chan(1, 1)
    xg, xg1, xl = "e" * g, "f" * (g + 1), "E" * LONG
    for x in (xg, xg1, xl):
        net.exchange(x, "direct")
    routes = [("", "k" * g), ("", "n" * (g + 1)), (xg, ""), (xg1, "r" * g), (xl, "R" * LONG), (xl, "s" * (g + 1))]
    tags = ["", "t", "u" * (g - 1), "v" * g, "w" * (g + 1), "T" * LONG]
    net.conn(2)
    for i, ((x, key), tag) in enumerate(zip(routes, tags)):
        q = key if x == "" else f"qf{i}"
        net.queue(q)
        if x:
            net.bind(q, x, key)
        net.chan(2, 1 + i)
        net.consume(2, 1 + i, q, tag, no_ack=i != 5)
    assert sorted(len(t) for t in tags) == [0, 1, g - 1, g, g + 1, LONG]
    assert {len(x) for x, _ in routes} == {0, g, g + 1, LONG} == {len(k) for _, k in routes}
    net.queue("qget")
    net.chan(3, 9)
    big = dict(HEADERS, message_id="i" * 30, content_type="application/octet-stream")
    assert len(encode_properties(big)) > 200 and encode_properties({}) == b"\x00\x00"
    i = 0
    for x, key in routes:
        for size in (0, 1, g - 1, g, g + 1):
            net.pub(1, 1, x, key, body_of(i, size), props=big if i % 2 else None)
            i += 1
    for _ in range(3):
        net.pub(1, 1, "", "qget", body_of(i, g + 1))
        i += 1
    net.get(3, 9, "qget")
    net.get(3, 9, "qget")
    st = net.step()
    assert st.n_deliv == 32 and st.n_runs == 8
    net.nack_requeue(2, 6, 3)
    net.get(3, 9, "qget")
    net.get(3, 9, "qget")
    st = net.step()
    assert st.n_deliv == 2 and len(net.expected[-1][3]) > 13 and net.expected[-1][3][-13:-11] == b"\x01\x00"
    flagged = [decode_method(f[7:-1]).redelivered for f in frames_of(net.expected[-1][2]) if f[0] == 1]
    assert flagged == [True]
    net.ack(2, 6, 0, multiple=True)
    net.step()
    assert net.step().n_live_msgs == 0
    return net.run(group=g, deliveries=34)


def sc_ref_edges(dp, lim, env):
    """Bodies of ref_min - 1 (inline) and ref_min bytes (referenced) alternate over consumers
    on three connections, so referenced and inline entries alternate along the gather table
    and every connection's offsets shift by the bodies taken out in front of it.  Connection
    2 has two returns and a confirm in front of its deliveries: the ``dst`` of its gather
    entries depends on both.  Connection 4 has frame-max 4096: a body of one byte more than
    its body frame holds is rendered inline for it and by reference for the others.  The
    step's rendered total is no multiple of 16, so the gather table starts at an offset
    rounded up."""
    rm = env.ref_min or 256
    net = Net(dp, env)
    net.chan(1, 1)
    net.chan(2, 1, confirm=True)
    net.chan(3, 1)
    net.conn(4, frame_max=4096)
    net.chan(4, 1)
    net.exchange("fan", "fanout")
    for c in (2, 3, 4):
        net.queue(f"e{c}")
        net.bind(f"e{c}", "fan", "")
        net.consume(c, 1, f"e{c}", f"ref-{c}")
    i = 0
    for rnd in range(3):
        for c in (2, 3, 4):
            net.pub(1, 1, "", f"e{c}", body_of(i, rm - 1 + (rnd + c) % 2))
            i += 1
    net.pub(1, 1, "fan", "", body_of(i, 4096 - 8 + 1))
    net.pub(1, 1, "fan", "", body_of(i + 1, 4096 - 8))
    net.pub(2, 1, "fan", "nobody", body_of(i + 2, rm), props={"reply_to": "x"})
    net.pub(2, 1, "", "nobody", body_of(i + 3, rm + 1), mandatory=True)
    net.pub(2, 1, "", "nobody", body_of(i + 4, 3), mandatory=True)
    st = net.step()
    by_ref = 4 + 2 + 3 + 3          # the alternating ones; 4089 on two connections; 4088 and 2's own on three
    assert st.n_deliv == 18 and st.n_returns == 2 and st.n_confirm_frames == 1
    if env.ref_min is not None:
        assert st.n_ref == by_ref and st.ref_bytes == 4 * rm + 2 * 4089 + 3 * 4088 + 3 * rm
        assert st.rendered % 16, st.rendered
    assert net.step().n_live_msgs == 0
    return net.run(n_ref=by_ref, rendered=st.rendered)


CAP_EGRESS = 1 << 16


def sc_cap_regions(dp, lim, env):
    """egress_cap 64 KB.  The budget bounds a step's deliveries, not its egress: connection 2
    gets 40 KB of returns and a confirm, and behind it connection 9 gets 52 KB of deliveries,
    most of them at offsets past egress_cap.  Every one of them must be rendered."""
    net = Net(dp, env)
    net.chan(1, 1)
    net.chan(2, 1, confirm=True)
    net.queue("cq")
    net.chan(9, 1)
    net.consume(9, 1, "cq", "capped")
    for i in range(40):
        net.pub(2, 1, "", "nobody", body_of(i, 900), mandatory=True)
    for i in range(200):
        net.pub(1, 1, "", "cq", body_of(100 + i, 200))
    st = net.step()
    out = net.expected[-1]
    assert st.n_deliv == 200 and st.n_returns == 40 and st.n_ref == 0
    assert len(out[9]) < CAP_EGRESS < len(out[2]) + len(out[9])
    assert net.step().n_live_msgs == 0
    return net.run(returns=len(out[2]), deliveries=len(out[9]), egress_cap=CAP_EGRESS)


# ================================================================ persist pack
PERSIST_MSG_MAX = 64


def sc_persist_pack(dp, lim, env):
    """Durable queues p1..p3 and a transient one, each with an auto-ack consumer, so every
    message slot is free again after its step and msg_max 64 hands them out again.  Persistent
    messages go to one durable queue, to three (a fanout: the bytes ride one record, the other
    two are headers only), to the transient queue (no record) and to a durable and the
    transient one; non-persistent messages go to durable queues (no record).
    Bodies of 0 to 9 bytes under one key: metadata + body covers every residue mod 8."""
    net = Net(dp, env)
    net.chan(1, 1)
    net.exchange("fan3", "fanout")
    net.exchange("mix", "fanout")
    for q in ("p1", "p2", "p3"):
        net.queue(q, durable=True)
        net.bind(q, "fan3", "")
    net.queue("tr")
    net.bind("p1", "mix", "")
    net.bind("tr", "mix", "")
    for i, q in enumerate(("p1", "p2", "p3", "tr")):
        net.chan(2, 1 + i)
        net.consume(2, 1 + i, q, "c-" + q)
    keep, once = {"delivery_mode": 2}, {"delivery_mode": 1}
    i, stored = 0, 0
    for k in range(6):
        for size in range(10):
            x, key = (("", "p2"), ("fan3", "any"), ("mix", "m"), ("", "tr"))[(size + k) % 4]
            net.pub(1, 1, x, key, body_of(i, size), props=keep)
            i += 1
        net.pub(1, 1, "fan3", "n", body_of(i, 5), props=once)
        net.pub(1, 1, "", "p1", body_of(i + 1, 6))
        i += 2
        net.step()
        stored += 12
    assert stored > PERSIST_MSG_MAX                       # more messages than slots: slots are taken again
    recs = [r for step in net.persist for r in step]
    sizes = {(len(r[2]) + len(r[3]) + len(r[4]) + len(r[5])) % 8 for r in recs}
    assert sizes == set(range(8)) and any(not r[5] for r in recs)
    assert {sum(1 for r in recs if r[6] == s) for s in {r[6] for r in recs}} == {1, 3}
    assert net.step().n_live_msgs == 0
    return net.run(records=len(recs), stored=stored)


def check_persist(run, outs, raw=False):
    """The step's persist records against the scenario's own expectation: one per durable
    queue a persistent message went to, with its queue position and its bytes.  ``raw`` (the
    HIP plane's packed buffer): size fields and offsets contiguous, persist_used their sum,
    each message's bytes in exactly one of its records, padded to a multiple of 8."""
    from chanamq_amd.engine.layout import PERSIST_HDR
    H = PERSIST_HDR.itemsize
    for k, (o, want) in enumerate(zip(outs, run.net.persist)):
        got = sorted((r[2], r[3], bytes(r[5]), bytes(r[6]), bytes(r[7]), bytes(r[8])) for r in o["persist"])
        assert got == sorted(r[:6] for r in want), f"step {k}: persist records"
        assert len({r[0] for r in o["persist"]}) == len({r[6] for r in want}), f"step {k}: message ids"
        if not raw:
            continue
        buf, off, carried, n = bytes(o["persist_raw"]), 0, defaultdict(int), 0
        assert len(buf) == o["counters"]["persist_used"] and o["counters"]["n_persist"] == len(want)
        while off < len(buf):
            h = struct.unpack_from("<qqQqIIHBBI", buf, off)
            mid, size, data = h[0], h[9], h[5] + h[6] + h[7] + h[8]
            assert data > 0 and size in (H, H + ((data + 7) & ~7)), f"step {k}: record {n} has size {size} for {data} bytes"
            carried[mid] += size > H
            off += size
            n += 1
        assert off == len(buf) and n == len(want), f"step {k}: {n} records in {off} of {len(buf)} bytes"
        assert set(carried.values()) <= {1}, f"step {k}: messages whose bytes ride {set(carried.values())} records"


# ---------------------------------------------------------------- the table
DELIV_BIG = dict(deliv_max=1 << 15, cmd_max=1 << 15, pair_max=1 << 15, msg_max=1 << 15, ucap=4096, seg_max=64)
WIDE_SMALL = dict(chpc=1, carry_cap=4096, ucap=16, cons_max=64, msg_max=1024, cmd_max=1024, deliv_max=1024,
                  ring_pool=1 << 16, default_queue_capacity=64, log_bytes=8 << 20, ingress_cap=1 << 20, egress_cap=1 << 20)
PERSIST_CFG = dict(persist=1, persist_max=4096, persist_bytes=8 << 20, msg_max=PERSIST_MSG_MAX)


def wide_cfg(lim):
    return dict(WIDE_SMALL, c_max=lim.CONN_LAYOUT_MAX + 2)


# (fn, engine overrides); every one is also compared byte by byte with the golden model
SCENARIOS = {
    "runs_lds": Scenario(sc_runs_lds, dict(cons_max=1024)),
    "deliv_passes": Scenario(sc_deliv_passes, DELIV_BIG),
    "deliv_passes_inline": Scenario(sc_deliv_passes, dict(DELIV_BIG, egress_ref=None)),
    "mixed_channel": Scenario(sc_mixed_channel, {}),
    "conn_regions_last": Scenario(lambda dp, lim, env: sc_conn_regions(dp, lim, env, True), {}),
    "conn_regions_silent": Scenario(lambda dp, lim, env: sc_conn_regions(dp, lim, env, False), {}),
    "conn_passes": Scenario(sc_conn_passes, dict(c_max=2 * CONN_PASS, chpc=2)),
    "return_frags": Scenario(sc_return_frags, {}),
    "return_flood": Scenario(sc_return_flood, {}),
    "confirm_channels": Scenario(sc_confirm_channels, {}),
    "deliver_fields": Scenario(sc_deliver_fields, {}),
    "ref_edges": Scenario(sc_ref_edges, {}),
    "ref_edges_inline": Scenario(sc_ref_edges, dict(egress_ref=None)),
    "cap_regions": Scenario(sc_cap_regions, dict(egress_cap=CAP_EGRESS)),
}
# their engine config depends on a limit of the build: made by wide_cfg(lim)
WIDE = Scenario(sc_conn_wide, None)
WIDE_BASE = Scenario(sc_conn_wide_base, dict(WIDE_SMALL, c_max=64))
PERSIST = Scenario(sc_persist_pack, PERSIST_CFG)
