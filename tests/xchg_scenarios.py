"""The sharded half of the data plane -- the cross-rank pack (k_pack_scan, k_pack / pack_one),
the import (k_import_route / import_one) and the host-injected import path behind
``Engine::restore`` (``GpuDataPlane.restore``, ``publish_host``, ``publish_to_queues``) -- at
the places where those kernels change path, in the style of ``route_scenarios`` and
``egress_scenarios``.

A scenario is ``(cl, lim, **params) -> Net``: it declares its topology and sends its traffic
through a ``Net`` over a ``LocalCluster`` (of golden planes or of ``GpuDataPlane``), which
applies both to the ranks and keeps its own record of them: which rank owns a queue, which
rank a connection sits on, every binding and every publish.  From that record alone

* ``Net.expected(k)`` renders what every connection must receive in step ``k`` with the host
  codec (``egress_scenarios.command``): returns in publish order, then one confirm frame per
  confirm-mode channel, then the deliveries of each of the connection's channels.  A queue's
  messages are ordered by (step of arrival, source rank, connection, publish order); a
  publish for a queue of another rank arrives ``exchange_lag`` steps later.  Routing is a
  dict for direct, a list for fanout and ``route_scenarios.topic_hit`` (a word-by-word walk)
  for topic, with the closure over exchange-to-exchange edges -- never the golden model or
  ``models/matcher.py``;
* ``Net.check_send_buffers`` compares what phase A packed -- the per-destination counts, the
  ``RDesc`` records and the payload in slot layout (``MF_SLOTFMT``: [exchange][key][props]
  padded to 16, then the body, the whole padded to 16) -- with a serialiser written here,
  before the exchange moves it, and the device's ``pub_rmask`` with the publishes the record
  sends to other ranks, index by index.

Byte equality with a single golden plane that holds every connection (``single_oracle``) and
with the golden cluster comes on top in the test files.  ``lim`` holds the kernels' limits as
the built extension exports them (``limits()``); every scenario asserts, while it is built,
the edge it sits on (``Net.placed`` records what was asserted) and the test files assert the
same from ``info()`` and the counters.
"""

from collections import defaultdict, namedtuple

import numpy as np

from chanamq_amd.engine.layout import MF_HAS_TS, MF_ONEQ, MF_PERSIST, MF_SLOTFMT, RDESC
from chanamq_amd.parallel.cluster import LocalCluster, _gpu_submit
from chanamq_amd.parallel.exchange import local_exchange
from chanamq_amd.protocol.codec import Method, encode_properties, render_command
from egress_scenarios import REPLY, body_of, command
from route_scenarios import bits_for, topic_hit
from sharded_scenarios import VH, Spec, apply

T0 = 1_800_000_000_000
REC = RDESC.itemsize
Limits = namedtuple("Limits", "PK_TILE WORLD_MAX PUB_QC SORT_ONEPASS_BITS")
P = namedtuple("P", "step rank conn ch seq x key props body routed queues ret lost")
NO_PROPS = {}
PERSISTENT = {"delivery_mode": 2}
STAMPED = {"timestamp": 1_700_000_123}
BOTH = {"delivery_mode": 2, "timestamp": 1_700_000_456}
SEG_PUBS = 1100       # publishes of one connection in one step: three frames each, below the frame scan's candidates


def limits():
    """The pack / import limits, from the built extension."""
    from chanamq_amd import ops
    m = ops.load()
    return Limits(*(int(getattr(m, k)) for k in Limits._fields))


def a16(n):
    return (n + 15) & ~15


def is_gpu(cl):
    return hasattr(cl[0], "eng")


def golden_kw(cfg):
    keys = ("c_max", "chpc", "q_max", "x_max", "cons_max", "ucap", "carry_cap", "default_queue_capacity", "deliver_cap",
            "ring_pool", "deliv_max", "egress_cap", "xfer_desc_max", "xfer_bytes", "persist", "persist_max")
    return {k: cfg[k] for k in keys if k in cfg}


def golden_cluster(cfg, world, lag=0):
    from chanamq_amd.engine.golden import GoldenDataPlane
    kw = golden_kw(cfg)
    return LocalCluster(lambda **k: GoldenDataPlane(exchange_lag=lag, **kw, **k), world)


def gpu_cluster(cfg, world, lag=0, graph=True):
    import torch

    from chanamq_amd.engine.dataplane import GpuDataPlane
    torch.cuda.set_device(0)
    return LocalCluster(lambda **k: GpuDataPlane(graph=graph, exchange_lag=lag, **cfg, **k), world)


# ---------------------------------------------------------------- one lockstep step
def cluster_step(cl, inputs, now_ms, after_pack=None):
    """``LocalCluster.step`` with a look at the send buffers between phase A and the exchange
    (``after_pack``), and a world of one stepped on its own.  -> [(egress, counters)] by rank."""
    if cl.world == 1:
        return [_result(cl[0].step(inputs[0], now_ms=now_ms))]
    gpu = is_gpu(cl)
    tickets = []
    for r, p in enumerate(cl.planes):
        if gpu:
            tickets.append(_gpu_submit(p, inputs[r], now_ms))
        else:
            p.step_a(inputs[r], now_ms)
    failed = None
    if after_pack is not None:
        try:
            after_pack()
        except AssertionError as e:     # reported once the step is through: no rank is left in mid-step
            failed = e
    recv = local_exchange(cl.planes)
    out = []
    for r, p in enumerate(cl.planes):
        if gpu:
            if p.lag:
                p.set_import(recv[r])
            else:
                p.submit_b(recv[r])
            out.append(_result(p.finish(tickets[r])))
        else:
            out.append(_result(p.step_b(recv[r])))
    if failed is not None:
        raise failed
    return out


def _result(r):
    if isinstance(r, dict):
        return dict(r["egress"]), dict(r["counters"])
    return dict(r.egress), dict(r.counters)


# ---------------------------------------------------------------- the record
class Net:
    def __init__(self, cl, lim, step_ms=1):
        self.cl, self.lim, self.world, self.step_ms = cl, lim, cl.world, step_ms
        self.lag = 1 if cl.world > 1 and getattr(cl[0], "lag", False) else 0
        self.xtype, self.binds, self.xbinds = {}, defaultdict(list), defaultdict(list)
        self.owner, self.slot, self.qorder = {}, {}, []
        self.cons = {}                      # queue -> (conn, ch, first step it is served in)
        self.rank_of, self.chans, self.frame_max, self.confirm = {}, defaultdict(list), {}, []
        self.pubs, self.steps, self.cur = [], [], defaultdict(list)
        self.ops = defaultdict(list)        # step -> control calls made before it
        self.pack = set()                   # steps whose send buffers are compared
        self.sent = {}                      # step -> [[records to rank d] by rank] the scenario names
        self.counters = {}                  # (step, rank) -> {counter: value}
        self.placed = {}
        self.plain = True                   # nothing the single-plane oracle's ``apply`` cannot set up
        self.ucap = cl[0].info["ucap"] if is_gpu(cl) else cl[0].ucap
        self._free_cons = defaultdict(list)
        self._next_conn = 63
        self._routes = {}

    # ---- topology
    def exchange(self, name, type_):
        self.cl.replicate("declare_exchange", VH, name, type_)
        self.xtype[name] = type_

    def queue(self, name, owner, capacity=1 << 12, consume=True, slot=None, **kw):
        if self.world > 1:
            self.cl.shard_map.place(VH, name, owner)
        if slot is not None:     # slots are handed out from the end of the free list, on every rank alike
            self.plain = False
            for p in self.cl.planes:
                p._free_q.remove(slot)
                p._free_q.append(slot)
        if kw:
            self.plain = False
        got = self.cl.replicate("declare_queue", VH, name, capacity=capacity, **kw)
        assert len(set(got)) == 1 and (slot is None or got[0] == slot), got
        self.owner[name], self.slot[name] = owner, got[0]
        self.qorder.append((name, owner, capacity))
        if consume:
            self.consume(name)
        return got[0]

    def bind(self, q, x, key=""):
        self.cl.replicate("bind", VH, q, x, key)
        self.binds[x].append((q, key.encode()))
        self._routes.clear()

    def xbind(self, dst, src, key=""):
        self.plain = False
        self.cl.replicate("bind_exchange", VH, dst, src, key)
        self.xbinds[src].append((dst, key.encode()))
        self._routes.clear()

    def open(self, conn, rank, ch=1, confirm=False, frame_max=None):
        dp = self.cl[rank]
        if conn not in self.rank_of:
            if frame_max is None:
                dp.open_connection(conn, VH)
            else:
                self.plain = False
                dp.open_connection(conn, VH, frame_max=frame_max)
                self.frame_max[conn] = frame_max
            self.rank_of[conn] = rank
        assert self.rank_of[conn] == rank
        if ch not in self.chans[conn]:
            dp.open_channel(conn, ch)
            self.chans[conn].append(ch)
        if confirm:
            dp.confirm_select(conn, ch)
            self.confirm.append((conn, ch))

    def consume(self, q, conn=None, ch=None, at_step=0):
        """A no-ack consumer of ``q`` on its owner, tag = the queue's name, one per channel
        (``at_step`` > 0: attached by a control call before that step)."""
        rank = self.owner[q]
        if conn is None:
            if not self._free_cons[rank]:
                self._free_cons[rank] = [(self._next_conn, c) for c in range(1, 9)]
                self._next_conn -= 1
            conn, ch = self._free_cons[rank].pop(0)
        assert conn not in self.rank_of or self.rank_of[conn] == rank
        call = lambda: (self.open(conn, rank, ch), self.cl[rank].consume(conn, ch, VH, q, q, no_ack=True))
        if at_step:
            self.plain = False
            self.ops[at_step].append(call)
        else:
            call()
        self.cons[q] = (conn, ch, at_step)

    # ---- brute-force routing
    def _match(self, x, kb):
        t = self.xtype[x]

        def hit(k):
            return True if t == "fanout" else k == kb if t == "direct" else topic_hit(k, kb)
        return {q for q, k in self.binds[x] if hit(k)}, {d for d, k in self.xbinds[x] if hit(k)}

    def route(self, x, key):
        """Queue names a publish to ``x`` with ``key`` reaches (the closure over the exchange-to-
        exchange edges, every exchange matched once), by slot; None for an unknown exchange."""
        if x not in self.xtype:
            return None
        got = self._routes.get((x, key))
        if got is None:
            seen, todo, hitq = {x}, [x], set()
            while todo:
                qs, xs = self._match(todo.pop(), key.encode())
                hitq |= qs
                for d in sorted(xs - seen):
                    seen.add(d)
                    todo.append(d)
            got = self._routes[(x, key)] = sorted(hitq, key=self.slot.get)
        return got

    # ---- traffic
    def pub(self, conn, x, key, size=0, props=NO_PROPS, mandatory=False, immediate=False, ch=1, lost=()):
        """One publish into the step under construction; what it must lead to is worked out
        here.  ``lost``: queues it is routed to that will not deliver it (the scenario says why)."""
        rank = self.rank_of[conn]
        routed = self.route(x, key)
        ret, queues = 0, routed
        if not routed:
            routed = queues = []
            ret = 312 if mandatory else 0
        elif immediate and all(self.owner[q] == rank for q in routed) and not any(q in self.cons for q in routed):
            ret, queues = 313, []
        i = len(self.pubs)
        body = body_of(i, size)
        p = P(len(self.steps), rank, conn, ch, i, x, key, props, body, routed, queues, ret, frozenset(lost))
        self.pubs.append(p)
        m = Method("basic.publish", exchange=x, routing_key=key, mandatory=mandatory, immediate=immediate)
        self.cur[conn].append(render_command(ch, m, props, body, self.frame_max.get(conn, 131072)))
        return p

    def step(self, pack=False, sent=None, **counters):
        """Close the step under construction.  ``pack``: compare its send buffers; ``sent``:
        {rank: [records to each rank]} the scenario names; ``counters``: {name: [by rank]}."""
        k = len(self.steps)
        if pack:
            self.pack.add(k)
        if sent is not None:
            self.sent[k] = sent
        for c, by_rank in counters.items():
            for r, v in enumerate(by_rank):
                self.counters.setdefault((k, r), {})[c] = v
        self.steps.append({c: b"".join(v) for c, v in self.cur.items()})
        self.cur = defaultdict(list)

    def drain(self):
        """The empty steps that hand over what a lagged exchange still holds and deliver every
        queue's backlog (a channel takes ``ucap`` deliveries a step)."""
        for _ in range(1 + self.lag):
            self.step()
        while self._simulate(len(self.steps))[1]:
            self.step()

    def now(self, k):
        return T0 + k * self.step_ms

    # ---- what every connection must receive
    def remote_ranks(self, p):
        return sorted({self.owner[q] for q in p.routed} - {p.rank}) if not p.ret else []

    def arrival(self, p, q):
        return p.step + (self.lag if self.owner[q] != p.rank else 0)

    def _simulate(self, nsteps):
        """({step: {conn: {ch: [bytes]}}} of every consumer over ``nsteps`` steps, messages left):
        a queue is a list in arrival order, its consumer's channel takes ``ucap`` a step, tags
        count from 1 per channel."""
        out = defaultdict(lambda: defaultdict(lambda: defaultdict(list)))
        left = 0
        for q, (conn, ch, first) in self.cons.items():
            mine = sorted((self.arrival(p, q), p.rank, p.conn, p.seq, p)
                          for p in self.pubs if q in p.queues and q not in p.lost)
            tag = i = 0
            for k in range(first, nsteps):
                room = self.ucap
                while i < len(mine) and mine[i][0] <= k and room:
                    p = mine[i][4]
                    tag, i, room = tag + 1, i + 1, room - 1
                    m = Method("basic.deliver", consumer_tag=q, delivery_tag=tag, redelivered=False, exchange=p.x,
                               routing_key=p.key)
                    out[k][conn][ch].append(command(ch, m, p.props, p.body, self.frame_max.get(conn, 131072)))
            left += len(mine) - i
        return out, left

    def deliveries(self):
        out, left = self._simulate(len(self.steps))
        assert not left, f"the scenario ends with {left} messages still queued"
        return out

    def expected(self):
        """[{conn: bytes}] per step: returns, confirms, deliveries by channel in opening order."""
        want = [defaultdict(bytes) for _ in self.steps]
        for p in self.pubs:
            if p.ret:
                m = Method("basic.return", reply_code=p.ret, reply_text=REPLY[p.ret], exchange=p.x, routing_key=p.key)
                want[p.step][p.conn] += command(p.ch, m, p.props, p.body, self.frame_max.get(p.conn, 131072))
        upto = defaultdict(int)
        for k in range(len(self.steps)):
            for conn, ch in sorted(self.confirm, key=lambda c: (c[0], self.chans[c[0]].index(c[1]))):
                n = sum(1 for p in self.pubs if (p.step, p.conn, p.ch) == (k, conn, ch))
                if n:
                    upto[(conn, ch)] += n
                    want[k][conn] += render_command(ch, Method("basic.ack", delivery_tag=upto[(conn, ch)], multiple=n > 1))
        for k, conns in self.deliveries().items():
            assert k < len(self.steps), f"the scenario ends before step {k} delivers"
            for conn, chs in conns.items():
                for ch in self.chans[conn]:
                    want[k][conn] += b"".join(chs.get(ch, ()))
        return [{c: b for c, b in w.items() if b} for w in want]

    # ---- what phase A must have packed
    def packed(self, k, rank):
        """[[(RDesc fields, meta bytes, body)] for each destination] of rank ``rank``'s step k,
        by this module's serialiser."""
        dp = self.cl[rank]
        out = [[] for _ in range(self.world)]
        off = [0] * self.world
        for p in sorted((p for p in self.pubs if p.step == k and p.rank == rank), key=lambda p: (p.conn, p.seq)):
            dests = self.remote_ranks(p)
            rq = [q for q in p.routed if self.owner[q] != rank]
            pb = encode_properties(p.props)
            meta = p.x.encode() + p.key.encode() + pb
            exp = p.props.get("expiration")
            ts = p.props.get("timestamp")
            flags = MF_SLOTFMT | (MF_PERSIST if p.props.get("delivery_mode") == 2 else 0) | (MF_HAS_TS if ts else 0)
            for d in dests:
                f = dict(pay_off=off[d], body_len=len(p.body), props_len=len(pb), exch=dp.exchanges[(VH, p.x)].slot,
                         flags=flags | (MF_ONEQ if len(rq) == 1 else 0), ex_len=len(p.x), rk_len=len(p.key),
                         expire_ms=self.now(k) + int(exp) if exp else 0, ts_ms=ts * 1000 if ts else 0,
                         tq=self.slot[rq[0]] if len(rq) == 1 else 0)
                out[d].append((f, meta, p.body))
                off[d] += a16(a16(len(meta)) + len(p.body))
        return out, off

    def rmasks(self, k, rank):
        """The remote-owner mask of every publish of rank ``rank``'s step k, in publish order."""
        mine = sorted((p for p in self.pubs if p.step == k and p.rank == rank), key=lambda p: (p.conn, p.seq))
        return [sum(1 << d for d in self.remote_ranks(p)) for p in mine]

    def check_send_buffers(self, k):
        """Phase A of step k on the device against ``packed``: counts, records, payload at the
        slot offsets (padding not compared) and the per-publish remote masks."""
        for rank, dp in enumerate(self.cl.planes):
            want, nbytes = self.packed(k, rank)
            cnt = list(dp.pending_send_counts())
            W = self.world
            assert cnt[:W] == [len(w) for w in want], f"step {k} rank {rank}: records by destination {cnt[:W]}"
            assert cnt[W:2 * W] == nbytes, f"step {k} rank {rank}: bytes by destination {cnt[W:2 * W]}, expected {nbytes}"
            n = sum(cnt[:W])
            desc = dp.xfer_send_desc()[:n * REC].cpu().numpy().view(RDESC)
            pay = dp.xfer_send_pay()[:sum(nbytes)].cpu().numpy().tobytes()
            i = base = 0
            for d in range(W):
                for j, (f, meta, body) in enumerate(want[d]):
                    got = {name: int(desc[i][name]) for name in f}
                    assert got == f, f"step {k} rank {rank} -> {d} record {j}: {got}, expected {f}"
                    o = base + f["pay_off"]
                    assert pay[o:o + len(meta)] == meta, f"step {k} rank {rank} -> {d} record {j}: exchange / key / props"
                    o += a16(len(meta))
                    assert pay[o:o + len(body)] == body, f"step {k} rank {rank} -> {d} record {j}: body"
                    i += 1
                base += nbytes[d]
            masks = self.rmasks(k, rank)
            if masks:
                got = np.frombuffer(dp.eng.download("pub_rmask", 0, 4 * len(masks)), np.uint32).tolist()
                bad = [i for i, (a, b) in enumerate(zip(got, masks)) if a != b]
                assert not bad, f"step {k} rank {rank}: remote masks differ at publishes {bad[:8]}"

    def to_spec(self):
        """The same topology and traffic as a ``sharded_scenarios.Spec`` (for the oracle)."""
        assert self.plain
        s = Spec()
        s.exchanges = list(self.xtype.items())
        s.queues = list(self.qorder)
        s.binds = [(q, x, k.decode()) for x, bs in self.binds.items() for q, k in bs]
        for conn, rank in self.rank_of.items():
            s.conn(rank, conn, *self.chans[conn])
        s.confirms = list(self.confirm)
        s.consumers = [(conn, ch, q, q, True) for q, (conn, ch, _) in self.cons.items()]
        s.steps = list(self.steps)
        return s


# ---------------------------------------------------------------- runner and judges
def run_net(net, pack=True):
    """Drive the cluster through the steps -> [{'egress': {conn: bytes}, 'counters': [by rank],
    'sent': [send counts by rank]}]; on the device the named steps' send buffers are compared."""
    cl, outs = net.cl, []
    for k, st in enumerate(net.steps):
        for call in net.ops.get(k, ()):
            call()
        inputs = [{c: b for c, b in st.items() if net.rank_of[c] == r} for r in range(net.world)]
        sent = []

        def after_pack():
            sent.extend(list(p.pending_send_counts()) for p in cl.planes)
            if pack and is_gpu(cl) and k in net.pack:
                net.check_send_buffers(k)
        res = cluster_step(cl, inputs, net.now(k), after_pack)
        merged = {}
        for eg, _ in res:
            assert not set(eg) & set(merged)
            merged.update(eg)
        outs.append(dict(egress=merged, counters=[c for _, c in res], sent=sent))
    return outs


def first_diff(a, b):
    n = min(len(a), len(b))
    return next((i for i in range(n) if a[i] != b[i]), n)


def check_run(net, outs, only=None):
    """``egress[conn] == expected[conn]`` for every connection and step; the send counts and
    the counters the scenario names (``only``: those this plane keeps)."""
    want = net.expected()
    assert len(outs) == len(want)
    for k, (o, w) in enumerate(zip(outs, want)):
        got = {c: b for c, b in o["egress"].items() if b}
        for c in sorted(set(got) | set(w)):
            g, e = got.get(c, b""), w.get(c, b"")
            assert g == e, (f"step {k} conn {c} (rank {net.rank_of.get(c)}): {len(g)} bytes, expected {len(e)}, "
                            f"first difference at {first_diff(g, e)}")
        if k in net.sent and net.world > 1:
            W = net.world
            for r, by_dest in net.sent[k].items():
                assert o["sent"][r][:W] == by_dest, f"step {k} rank {r}: sent {o['sent'][r][:W]}, expected {by_dest}"
        for (kk, r), named in net.counters.items():
            if kk == k:
                for c, v in named.items():
                    if only is None or c in only:
                        assert o["counters"][r].get(c, 0) == v, f"step {k} rank {r}: {c} = {o['counters'][r].get(c, 0)}, expected {v}"


def assert_same_egress(a, b, what):
    assert len(a) == len(b)
    for k, (x, y) in enumerate(zip(a, b)):
        x = {c: v for c, v in x.items() if v}
        y = {c: v for c, v in y.items() if v}
        assert set(x) == set(y), f"{what} step {k}: connections {sorted(x)} / {sorted(y)}"
        for c in x:
            assert x[c] == y[c], f"{what} step {k} conn {c}: first difference at {first_diff(x[c], y[c])}"


def single_oracle(net, cfg):
    """One golden plane holding every connection, connection ids renamed so that their order
    is (rank, connection): the cross-rank enqueue order of the sharded plane.  Exact only
    without a lag (a lagged exchange delivers a remote publish a step later)."""
    from chanamq_amd.engine.golden import GoldenDataPlane
    assert net.lag == 0
    spec = net.to_spec()
    remap = {c: r * 64 + c for c, r in net.rank_of.items()}
    back = {v: k for k, v in remap.items()}
    dp = GoldenDataPlane(**dict(golden_kw(cfg), c_max=64 * net.world))
    apply(dp, spec, conn_map=remap)
    out = []
    for k, st in enumerate(spec.steps):
        eg = dp.step({remap[c]: b for c, b in st.items()}, now_ms=net.now(k))["egress"]
        out.append({back[c]: b for c, b in eg.items()})
    return out


def check_empty(net):
    """Once the run is over every queue with a consumer is empty on its owner, and no rank
    holds a message of a queue it does not own, consumer or not: each owner enqueued only its
    own queues."""
    for q, slot in net.slot.items():
        for r, p in enumerate(net.cl.planes):
            n = p.message_count(slot)
            if net.owner[q] != r:
                assert n == 0, f"rank {r} holds {n} messages of queue {q}, which rank {net.owner[q]} owns"
            elif q in net.cons:
                assert n == 0, f"queue {q} on rank {r} still holds {n} messages"


# ================================================================ the scenarios
def sized(j):
    """(key, props, body size) of the j-th record-bound publish: over 16 in a row the key
    length and the body size take every residue mod 16; an empty key, a 255-byte key and an
    empty body come round too."""
    klen = 255 if j % 37 == 5 else 0 if j % 37 == 6 else j % 16 + 16 * (j % 3)
    props = (NO_PROPS, PERSISTENT, STAMPED, BOTH)[(j // 16) % 4]
    size = 0 if j % 41 == 7 else (j * 7) % 16 + 16 * (j % 5)
    return "k" * klen, props, size


def spread(n):
    """The producer connection (1, 2, ..) of publish i of a step, keeping (connection,
    position) = publish order."""
    return lambda i: 1 + i // SEG_PUBS


REMOTE_AT = (0, 63, 64, 1022, 1023, 1024, 1025, 2047, 2048)


def sc_tile_edges(cl, lim, prod=0, pub_max=4096):
    """One producer rank; fanout exchanges to a local queue (xl), to one queue on another rank
    (xa; xb on the third rank), to queues on two ranks (xab; at world 2 one remote and one
    local) and to nothing (xn).  Steps of 1 .. pub_max publishes, most of them local or
    unroutable, the record-bound ones at the first / last lane of a wave and of a tile and at
    the step's last publish; then a full wave and a full tile for one destination, and a wave
    alternating between two."""
    T, W = lim.PK_TILE, cl.world
    net = Net(cl, lim)
    others = [r for r in range(W) if r != prod]
    A, B = others[0], others[1] if W > 2 else None
    for x in ("xl", "xa", "xb", "xab", "xn"):
        net.exchange(x, "fanout")
    net.queue("ql", prod), net.bind("ql", "xl")
    net.queue("qa", A), net.bind("qa", "xa")
    net.queue("qa2", A), net.bind("qa2", "xab")
    if B is not None:
        net.queue("qb", B), net.bind("qb", "xb")
        net.queue("qb2", B), net.bind("qb2", "xab")
    else:
        net.queue("ql2", prod), net.bind("ql2", "xab"), net.bind("ql", "xb")   # (xb: local at world 2)
    nconn = -(-pub_max // SEG_PUBS)
    for c in range(nconn):
        net.open(1 + c, prod)
    counts = (1, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1, pub_max)
    assert T == 1024 and pub_max == 4 * T, "the publish counts and REMOTE_AT below are written for 1024-publish tiles"
    j = 0
    cyc = ("xa", "xb", "xab")

    def fill(n, pick):
        nonlocal j
        conn = spread(n)
        for i in range(n):
            x = pick(i)
            if x in cyc:
                key, props, size = sized(j)
                j += 1
                net.pub(conn(i), x, key, size, props)
            else:
                net.pub(conn(i), x, "k", 8 if x == "xl" else 0)
    for n in counts:
        at = {i for i in REMOTE_AT if i < n} | {n - 1}
        fill(n, lambda i: cyc[i % 3] if i in at else "xl" if i % 5 == 0 else "xn")
        net.step(pack=True, n_pubs=[n if r == prod else 0 for r in range(W)])
    fill(3 * 64, lambda i: "xa" if 64 <= i < 128 else "xn")                               # a full wave, one destination
    net.step(pack=True, sent={prod: [64 if r == A else 0 for r in range(W)]})
    fill(2 * T + 1, lambda i: "xa" if T <= i < 2 * T else "xl" if i % 5 == 0 else "xn")   # a full tile
    net.step(pack=True, sent={prod: [T if r == A else 0 for r in range(W)]})
    fill(3 * 64, lambda i: ("xa", "xb")[i % 2] if 64 <= i < 128 else "xn")                # a wave, two destinations in turn
    net.step(pack=True, sent={prod: [32 if r in (A, B) else 0 for r in range(W)]})
    net.drain()
    bound = [p for p in net.pubs if net.remote_ranks(p)]
    metas = {(len(p.x) + len(p.key) + len(encode_properties(p.props))) % 16 for p in bound}
    assert metas == set(range(16)) and {len(p.body) % 16 for p in bound} == set(range(16))
    assert any(not p.body for p in bound) and {0, 255} <= {len(p.key) for p in bound}
    net.placed = dict(tiles=[-(-n // T) for n in counts], bound=len(bound))
    return net


MANY_CONNS = 26


def sc_many_tiles(cl, lim):
    """65 * PK_TILE + 1 minimal publishes in one step of rank 0: 66 tiles, so the last tile's
    prefix loop (64 tiles a round) goes round twice and ``carry`` takes the first round's totals
    to tiles 64 and 65.  Record-bound publishes sit in tiles 0, 63, 64 and 65 only; the rest are
    unroutable and not mandatory, so nothing is stored for them."""
    T = lim.PK_TILE
    n = 65 * T + 1
    net = Net(cl, lim)
    net.exchange("xa", "fanout"), net.exchange("xn", "fanout")
    net.queue("qa", 1), net.bind("qa", "xa")
    per = -(-n // MANY_CONNS)
    assert 2 * per + 64 < 8192, "a connection's frames stay below the frame scan's candidate slots"
    for c in range(MANY_CONNS):
        net.open(c, 0)
    at = {t * T + i for t in (0, 63, 64, 65) for i in (0, 1, 63, 64, T - 1) if t * T + i < n}
    assert max(at) == n - 1 and len(at) == 16
    j = 0
    for i in range(n):
        if i in at:
            key, props, size = sized(j)
            j += 1
            net.pub(i // per, "xa", key, size + 1, props)
        else:
            net.pub(i // per, "xn", "")
    net.step(pack=True, sent={0: [0, len(at)]}, n_pubs=[n, 0])
    net.drain()
    net.placed = dict(tiles=-(-n // T), bound=sorted(at))
    assert net.placed["tiles"] == 66
    return net


def sc_world_wide(cl, lim, high_slots=False):
    """Every rank owns a queue of a fanout exchange (every bit of the remote mask), a queue
    with a direct key of its own (MF_ONEQ to every destination) and a queue of a topic exchange
    whose three patterns reach 2, 3 and W - 1 ranks.  One producer on every rank publishes to
    all of them, in two steps: every queue gets messages from every source, ranks below and above
    its owner, and with a lag a step's own publishes are enqueued among the imports of the step before.
    ``high_slots``: the queues sit at the top of a wide queue table (a pair key wider than 8
    bits)."""
    W = cl.world
    net = Net(cl, lim)
    net.exchange("fx", "fanout"), net.exchange("dx", "direct"), net.exchange("tx", "topic")
    two, three, most = {1, W // 2}, {0, W // 2, W - 1}, set(range(W)) - {2}
    q_max = cl[0].q_max
    slots = iter([q_max + 6 - 7 * i if i % 2 else 3 * i for i in range(3 * W)]) if high_slots else None
    for r in range(W):
        for i, name in enumerate((f"f{r}", f"d{r}", f"t{r}")):
            net.queue(name, r, consume=False, slot=next(slots) if slots else None)
            net.consume(name, 32 + r, 1 + i)
        net.bind(f"f{r}", "fx"), net.bind(f"d{r}", "dx", f"key.{r}")
        for pat, ranks in (("two.*", two), ("three.*", three), ("most.#", most)):
            if r in ranks:
                net.bind(f"t{r}", "tx", pat)
    for r in range(W):
        net.open(r, r)
    for rnd in range(2):     # twice: with a lag the second step's own publishes meet the first step's imports
        for r in range(W):
            net.pub(r, "fx", "any", 20 + r)
            for d in range(W):
                net.pub(r, "dx", f"key.{d}", 5 + d + rnd, PERSISTENT if d % 2 else NO_PROPS)
            net.pub(r, "tx", "two.a", 33), net.pub(r, "tx", "three.b", 17), net.pub(r, "tx", "most.c.d", 64)
            net.pub(r, "fx", "", 0)
        net.step(pack=True, sent={r: [3 + (d in two) + (d in three) + (d in most) if d != r else 0 for d in range(W)]
                                  for r in range(W)})
    net.drain()
    mid = W // 2
    srcs = {p.rank for p in net.pubs if f"t{mid}" in p.queues}
    assert min(srcs) < mid < max(srcs) and len(srcs) == W
    net.placed = dict(world=W, key_bits=bits_for(q_max) + 1, slots=sorted(net.slot.values()))
    return net


def sc_oneq_paths(cl, lim):
    """World 3, producers on ranks 0 and 1.  For a direct, a fanout and a topic exchange: a
    publish with exactly one remote queue (MF_ONEQ: the queue travels in ``tq``), one remote
    and one local, two remote on one rank, two remote on two ranks, more than PUB_QC local and
    one remote, and a publish that reaches its one remote queue over an exchange-to-exchange
    edge.  The topic keys have 1 to 9 words, the patterns '#', and an empty and a 255-byte key
    are among them: where the owner matches again (two remote queues) it does so with the key
    vector ``import_one`` builds."""
    assert cl.world == 3
    net = Net(cl, lim)
    nloc = lim.PUB_QC + 1
    for i in range(nloc):
        net.queue(f"loc{i}", 0)
    long_key = "c." + "w" * 253
    plan = {}
    for t in ("direct", "fanout", "topic"):
        s = t[0]
        sets = dict(a=[(f"{s}a", 1)], b=[(f"{s}b1", 2), (f"{s}b0", 0)], c=[(f"{s}c1", 1), (f"{s}c2", 1)],
                    d=[(f"{s}d1", 1), (f"{s}d2", 2)], e=[(f"{s}e", 2)] + [(f"loc{i}", 0) for i in range(nloc)],
                    f=[(f"{s}f", 2)])
        pats = dict(a="a1.only", b="b.*", c="c.#", d="#.d", e="e.many", f="f.#")
        keys = dict(a=["a1.only"], b=["b.x"], e=["e.many"], f=["f.x.y"],
                    c=["c"] + ["c." + ".".join(f"w{i}" for i in range(n)) for n in range(1, 9)] + [long_key],
                    d=["d"] + [".".join(f"v{i}" for i in range(n)) + ".d" for n in range(1, 9)] + [""])
        for case, qs in sets.items():
            if case == "f":
                x = f"hop{s}"
                net.exchange(x, t)
            elif t == "fanout":
                x = f"x{s}{case}"
                net.exchange(x, "fanout")
            else:
                x = f"x{s}"
                if x not in net.xtype:
                    net.exchange(x, t)
            for q, owner in qs:
                if q not in net.slot:
                    net.queue(q, owner)
            if case == "f":    # the entry exchange has nothing but an edge to a leaf that holds the queue
                leaf = f"leaf{s}"
                net.exchange(leaf, "fanout")
                net.bind(qs[0][0], leaf)
                key = {"direct": "f.x.y", "fanout": "", "topic": "f.#"}[t]
                net.xbind(leaf, x, key)
            else:
                for q, _ in qs:
                    net.bind(q, x, "" if t == "fanout" else pats[case] if t == "topic" else keys[case][0])
                    if t == "topic" and case == "d":
                        net.bind(q, x, "")      # the empty key is one empty word: only the empty pattern takes it
            plan[(t, case)] = (x, keys[case] if t == "topic" else keys[case][:1])
    net.open(1, 0), net.open(2, 1)
    j = 0
    for conn in (1, 2):
        for (t, case), (x, keys) in plan.items():
            for key in keys:
                _, props, size = sized(j)
                j += 1
                net.pub(conn, x, key, size, props)
    net.step(pack=True)
    net.drain()
    from0 = [p for p in net.pubs if p.rank == 0]
    nrem = lambda p: sum(1 for q in p.routed if net.owner[q] != p.rank)
    assert {nrem(p) for p in from0} == {1, 2} and any(nrem(p) == 1 and len(p.routed) > lim.PUB_QC for p in from0)
    assert any(len(p.key.split(".")) == 9 for p in net.pubs if p.x == "xt") and any(p.key == "" and p.routed for p in net.pubs)
    net.placed = dict(oneq=sum(1 for p in net.pubs if nrem(p) == 1), rematched=sum(1 for p in net.pubs if nrem(p) > 1))
    return net


FM_SMALL = 4096


def sc_record_fields(cl, lim):
    """World 2, every field of a record: persistent and transient, with and without a
    timestamp, an expiration that outlives the exchange and one that has passed when the owner
    looks at its queue's head (only a lagged exchange takes that long), the smallest
    properties and the largest a frame-max of 4096 allows, mandatory with only a remote queue
    (no return), immediate with only a remote queue that has no consumer (never 313),
    mandatory unroutable (312, nothing packed), a confirm-mode channel whose publishes all go
    to the other rank, and a remote queue at capacity."""
    assert cl.world == 2
    net = Net(cl, lim, step_ms=5)
    net.exchange("rx", "direct")
    net.queue("qr", 1), net.bind("qr", "rx", "r")
    net.queue("qi", 1, consume=False), net.bind("qi", "rx", "i")
    net.queue("qfull", 1, capacity=4, max_capacity=4, consume=False), net.bind("qfull", "rx", "full")
    net.queue("ql", 0), net.bind("ql", "rx", "l")
    net.open(1, 0), net.open(2, 0, confirm=True), net.open(3, 0, frame_max=FM_SMALL)
    # the head of qr at its first arrival: gone if that is a step later
    short = dict(PERSISTENT, expiration="3")
    net.pub(1, "rx", "r", 40, short, lost=("qr",) if net.lag else ())
    for props in (NO_PROPS, PERSISTENT, STAMPED, BOTH, dict(BOTH, expiration="60000")):
        net.pub(1, "rx", "r", 24, props)
    pad = FM_SMALL - 8 - 12 - len(encode_properties({"headers": {"k": ""}}))
    big = {"headers": {"k": "v" * pad}}
    assert len(encode_properties(big)) == FM_SMALL - 8 - 12
    net.pub(3, "rx", "r", 100, big)
    net.pub(1, "rx", "r", 10, mandatory=True)
    net.pub(1, "rx", "i", 11, immediate=True)
    net.pub(1, "rx", "none", 12, mandatory=True)
    net.pub(1, "rx", "none", 13)
    net.pub(1, "rx", "l", 14)
    for i in range(3):
        net.pub(2, "rx", "r", 30 + i, PERSISTENT)
    for i in range(6):       # a ring of 4 on the other rank: the last two are dropped there, the confirm is an Ack
        net.pub(2, "rx", "full", 50 + i, lost=("qfull",) if i >= 4 else ())
    net.step(pack=True, sent={0: [0, 8 + 1 + 3 + 6]}, n_returns=[1, 0])
    net.step()
    net.step()
    net.consume("qfull", at_step=len(net.steps))
    net.consume("qi", at_step=len(net.steps))
    net.drain()
    ring_full = [0, 2]
    net.counters[(net.lag, 1)] = dict(n_ring_full=ring_full[1])
    net.placed = dict(ret=[p.ret for p in net.pubs if p.ret], full=ring_full)
    return net


HEAVY = 1025


def sc_step_sequence(cl, lim):
    """World 2: an empty step (tile 0 of k_pack_scan runs alone and publishes zero totals), a
    step of PK_TILE + 1 record-bound publishes, an empty one, one publish, an empty one.  The
    send counts go 0, n, 0, 1, 0 and nothing of the heavy step is seen again."""
    assert cl.world == 2 and HEAVY == lim.PK_TILE + 1
    net = Net(cl, lim)
    net.exchange("xa", "fanout"), net.exchange("xb", "fanout")
    net.queue("qa", 1), net.bind("qa", "xa")
    net.queue("qb", 0), net.bind("qb", "xb")
    net.open(1, 0), net.open(2, 0), net.open(3, 1)
    net.step(pack=True, sent={0: [0, 0], 1: [0, 0]})
    for i in range(HEAVY):
        key, props, size = sized(i)
        net.pub(1 + i // SEG_PUBS, "xa", key[:40], size, props)
    for i in range(3):
        net.pub(3, "xb", "back", 9)
    net.step(pack=True, sent={0: [0, HEAVY], 1: [3, 0]})
    net.step(pack=True, sent={0: [0, 0], 1: [0, 0]})
    net.pub(2, "xa", "one", 77, BOTH)
    net.step(pack=True, sent={0: [0, 1], 1: [0, 0]})
    net.step(pack=True, sent={0: [0, 0], 1: [0, 0]})
    net.drain()
    net.placed = dict(sent=[0, HEAVY, 0, 1, 0])
    return net


# ---- capacity: the send buffers
SEND_K, SEND_B = 8, 1024
SEND_CFG = dict(xfer_desc_max=SEND_K, xfer_bytes=SEND_B)
SEND_CASES = {"k_records": ([16] * SEND_K, True), "k_plus_1_records": ([16] * (SEND_K + 1), False),
              "b_bytes": ([SEND_B // 4 - 16] * 4, True), "b_plus_16_bytes": ([SEND_B // 4 - 16] * 3 + [SEND_B // 4 - 15], False)}


def sc_send_limits(cl, lim, case="k_records"):
    """World 2 with send buffers of SEND_K records and SEND_B bytes.  Every record's exchange,
    key and properties take 16 bytes, so a record is 16 + align16(body) bytes in the slot
    layout and in the model's: exactly SEND_K records and exactly SEND_B bytes pass and
    deliver everything; one record or 16 bytes more is refused."""
    sizes, fits = SEND_CASES[case]
    net = Net(cl, lim)
    net.exchange("sx", "fanout")
    net.queue("qs", 1), net.bind("qs", "sx")
    net.open(1, 0)
    key = "k" * (16 - 2 - len(encode_properties(NO_PROPS)))
    for size in sizes:
        net.pub(1, "sx", key, size)
    n, total = len(sizes), sum(a16(16 + size) for size in sizes)
    assert (n, total) in ((SEND_K, SEND_K * 32), (SEND_K + 1, (SEND_K + 1) * 32), (4, SEND_B), (4, SEND_B + 16)), (n, total)
    assert fits == (n <= SEND_K and total <= SEND_B)
    net.step(pack=fits, sent={0: [0, n]})
    net.drain()
    net.placed = dict(records=n, bytes=total, fits=fits)
    return net


# ---- capacity: the import buffers
RECV_MAX = 16
RECV_CFG = dict(import_max=RECV_MAX)


def sc_recv_limits(cl, lim):
    """World 3, rank 2 built to import RECV_MAX records a step: ranks 0 and 1 send it half of
    that each, and all of it is imported.  (The test file then hands rank 2 counts one above
    the limit with nothing copied, and runs the last step of this record after it.)"""
    assert cl.world == 3
    net = Net(cl, lim)
    net.exchange("vx", "fanout")
    net.queue("qv", 2), net.bind("qv", "vx")
    net.open(1, 0), net.open(2, 1)
    for i in range(RECV_MAX // 2):
        net.pub(1, "vx", "a", 20 + i), net.pub(2, "vx", "b", 40 + i)
    net.step(sent={0: [0, 0, RECV_MAX // 2], 1: [0, 0, RECV_MAX // 2]})
    net.drain()
    net.pub(1, "vx", "after", 5), net.pub(2, "vx", "after", 6)
    net.step(sent={0: [0, 0, 1], 1: [0, 0, 1]})
    net.drain()
    net.placed = dict(received=RECV_MAX, normal_again=len(net.steps) - 1 - (1 + net.lag))
    return net


SCENARIOS = {"tile_edges": sc_tile_edges, "many_tiles": sc_many_tiles, "world_wide": sc_world_wide,
             "oneq_paths": sc_oneq_paths, "record_fields": sc_record_fields, "step_sequence": sc_step_sequence,
             "send_limits": sc_send_limits, "recv_limits": sc_recv_limits}


# ================================================================ the host-injected import path
RESTORE_MAX = 64
RESTORE_BYTES = 8192
Item = namedtuple("Item", "queue mid ts expire ex rk props body persistent redelivered")


def restore_items(n, queue, first_id, big=False):
    """n store records for ``queue``: sizes over every residue mod 16, empty bodies, every
    combination of the persistent and redelivered flags; ``big``: bodies that make a chunk of
    RESTORE_MAX records pass RESTORE_BYTES."""
    out = []
    for i in range(n):
        key, props, size = sized(i)
        if big:
            size += 900
        out.append(Item(queue, first_id + i, 1_700_000_000_000 + i, 0, "rx", key[:60], props, body_of(first_id + i, size),
                        i % 2 == 1, i % 3 == 0))
    return out


def restore_wire(it, ch, tag):
    """The Basic.Deliver of a restored item, by the host codec."""
    m = Method("basic.deliver", consumer_tag=it.queue, delivery_tag=tag, redelivered=it.redelivered, exchange=it.ex,
               routing_key=it.rk)
    return command(ch, m, it.props, it.body)


def restore_tuple(it, slot):
    return (slot, it.mid, it.ts, it.expire, it.ex.encode(), it.rk.encode(), encode_properties(it.props), it.body,
            it.persistent, it.redelivered)


def restore_chunks(items):
    """The batches ``GpuDataPlane.restore`` must cut: at most RESTORE_MAX records, and payload
    (each record padded to 16) within RESTORE_BYTES."""
    chunks, cur, nb = [], 0, 0
    for it in items:
        b = a16(len(it.ex) + len(it.rk) + len(encode_properties(it.props)) + len(it.body))
        if cur and (cur == RESTORE_MAX or nb + b > RESTORE_BYTES):
            chunks.append(cur)
            cur = nb = 0
        cur += 1
        nb += b
    return chunks + [cur]
