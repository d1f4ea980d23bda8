"""The body tiers -- HBM log, pinned-host spill ring, cold store -- at their edges: k_spill /
spill_queue (also inside k_dequeue under stage_spill), spill_reserve and the ring's tail in
final_step, k_cold_pick / k_cold_commit / k_cold_scan / k_cold_in, and the q_cold_lim holds
in the dequeue, the TTL walk, trim_head and k_basic_get.

Where a body lives must be invisible to clients, so the golden model has no tiers and the
reference for every client-visible byte is the golden run of the same steps with the tier
operations left out.  A scenario is ``(dp, ctx) -> steps``; a step may carry

  ``__spill__``        dict(frac, hot) | dict(lim, hot): ``dp.spill`` / ``eng.spill``
  ``__stage_spill__``  dict(frac, hot, budget): ``eng.stage_spill`` (frac in 1/65536 of the log)
  ``__cold_out__``     dict(hot, max_n, max_bytes, frac): k_cold_pick, the store, k_cold_commit
  ``__cold_in__``      dict(window): ``dp.cold_in``
  ``__tier__``         ``fn(dp, ctx)``: device-state expectations (and whatever else only a
                       plane with tiers can do), after the four above

(each a dict or a list of dicts, applied in this order before the step) on a plane that has the
tiers; the golden plane ignores them.  ``__do__`` (``fn(dp)``: control operations), ``__ops__``
and ``__get__`` run on both.  Every result of a tier operation is appended to ``ctx.moved`` as
``(kind, bytes)``.  ``lockstep`` scenarios page cold bodies in before the step that is to
deliver them and are compared with the golden run step by step; the others (the hold itself,
page-in under a full ring) are compared by what each connection saw over the whole run, and
state what each step may deliver.

Tier configuration: log_block 64 KiB, log_bytes 1 MiB, spill_bytes 512 KiB -- the engine
accepts blocks that small.  A 4080-byte body behind the default exchange has a 4096-byte slot:
16 fill a block, 256 the log, 128 the ring.

Expected values come from the golden model (client bytes), the protocol (``CHECKS``) and
``RingModel``, a replica of the ring arithmetic written from dp_state.h / dataplane.hip:
spill_reserve pads to the wrap, never across it, and is full against the *lagged* tail (the
lowest of the last SPILL_LAG steps' tails and the current one); final_step advances the tail
block by block while the block's live bytes are 0, never into the head's block.  With equal
slots the ring's head, total and per-block live bytes and the bytes moved are deterministic
(which message gets which position is not: four waves race in spill_queue); with mixed sizes
only conservation is asserted.

Left out: ``min_used`` of k_cold_pick is only reachable through ``eng.side_cold_pick``, a side
operation that needs a step in flight to carry it (GpuBroker._side); between-steps calls pass 0."""

import os
import re
from collections import namedtuple

import numpy as np

from chanamq_amd.engine.traffic import ack_frame, publish_command
from chanamq_amd.protocol.codec import encode_properties
from consumer_scenarios import FM, body_of, nack, observe, open_ch, serial
from dp_scenarios import NOW, VH
from get_scenarios import decode_get, golden_plane, is_gpu, serve_gets, slot_bytes, step_out

Scenario = namedtuple("Scenario", "fn cfg now_step_ms lockstep kw")
LOG_BLOCK, LOG_BYTES, SPILL_BYTES = 64 << 10, 1 << 20, 512 << 10
TIER = dict(log_block=LOG_BLOCK, log_bytes=LOG_BYTES, spill_bytes=SPILL_BYTES)
SEG_SHIFT = 30          # dp_common.h COLD_SEG_SHIFT
ALL = 1 << 40           # "no limit" for max_bytes / lim_rel
SHORT = {"expiration": "1000"}
STEP_MS = 2000


def spill_lag():
    """SPILL_LAG of csrc/kernels/dp_state.h."""
    here = os.path.dirname(os.path.abspath(__file__))
    with open(os.path.join(here, "..", "csrc", "kernels", "dp_state.h")) as f:
        return int(re.search(r"#define\s+SPILL_LAG\s+(\d+)", f.read()).group(1))


SPILL_LAG = spill_lag()


def slot_of(rk, body, props=None, ex=""):
    return slot_bytes(ex.encode(), rk.encode() if isinstance(rk, str) else rk, encode_properties(props or {}), body)


S4K = 4096              # slot of a 4080-byte body (exchange "", a short key, no properties)
B4K = S4K - 16


def pubs(q, lo, hi, size, props=None):
    return b"".join(publish_command(1, "", q, body_of(q, i, size), props) for i in range(lo, hi))


# ---------------------------------------------------------------- the ring's arithmetic
class RingModel:
    def __init__(self, size=SPILL_BYTES, block=LOG_BLOCK, lag=SPILL_LAG):
        self.size, self.block, self.head, self.tail = size, block, 0, 0
        self.lag = [0] * lag
        self.live = [0] * (size // block)
        self.steps = 0

    def lagged_tail(self):
        return min([self.tail] + self.lag)

    def fits(self, sz, head=None, tail=None):
        """Where spill_reserve would put ``sz`` bytes, or None when the ring is full."""
        h = self.head if head is None else head
        tail = self.lagged_tail() if tail is None else tail
        phys = h % self.size
        if phys + sz > self.size:
            h += self.size - phys                     # pad to the wrap, never across it
        return None if h + sz - tail > self.size else h

    def reserve(self, sz):
        h = self.fits(sz)
        if h is None:
            return None
        self.head = h + sz
        self.live[(h // self.block) % len(self.live)] += sz
        return h

    def release(self, pos, sz):
        self.live[(pos // self.block) % len(self.live)] -= sz

    def end_step(self):
        """final_step: the tail over the blocks without live bytes, never into the head's."""
        st, sh = self.tail, self.head
        while st < sh:
            bi = st // self.block
            if bi == sh // self.block or self.live[bi % len(self.live)] > 0:
                break
            st = (bi + 1) * self.block
        self.tail = min(st, sh)
        self.lag[self.steps % len(self.lag)] = self.tail
        self.steps += 1


# ---------------------------------------------------------------- device state
def dev(dp, name, dtype="<u8"):
    return np.frombuffer(dp.eng.download(name), dtype).copy()


def dev1(dp, name):
    return int(dev(dp, name)[0])


def ring_state(dp):
    return dict(head=dev1(dp, "spill_head"), tail=dev1(dp, "spill_tail"), lag=[int(x) for x in dev(dp, "spill_tail_lag")],
                live=[int(x) for x in dev(dp, "spill_live", "<i8")])


def assert_ring(dp, ring):
    """The device's ring equals the replica: head, tail, lag history (as a multiset: the slot a
    step writes depends on the engine's step counter) and live bytes per block."""
    st = ring_state(dp)
    assert st["head"] == ring.head and st["tail"] == ring.tail, (st, ring.head, ring.tail)
    assert sorted(st["lag"]) == sorted(ring.lag), (st["lag"], ring.lag)
    assert st["live"] == ring.live, (st["live"], ring.live)


def cold_lim(dp, qname):
    return int(dev(dp, "q_cold_lim")[dp.queues[(VH, qname)].slot])


NOT_HELD = (1 << 64) - 1


def live_sums(dp):
    return dict(log=int(dev(dp, "log_live", "<i8").sum()), spill=int(dev(dp, "spill_live", "<i8").sum()),
                cold=int(dp.cold_live().sum()))


def cold_out(dp, store, hot=0, max_n=1 << 16, max_bytes=ALL, frac=1.0, commit=True):
    """``GpuDataPlane.cold_out`` with the batch's record cap exposed; returns the records of the
    pick (those cut by max_bytes carry bytes 0) with their store offsets."""
    from chanamq_amd.store.cold import COLD_REC
    lim = int(frac * dp.info["spill_bytes"])
    recs = np.frombuffer(dp.eng.cold_pick(int(hot), lim, int(max_n), int(max_bytes)), COLD_REC).copy()
    kept = dp._cold_store(store, recs.copy())
    if kept is not None and commit:
        dp.eng.cold_commit(kept)
    return recs, kept


class Ctx:
    """What a run carries beside the plane: the cold store, the ring replica, the results of the
    tier operations and the clock of the last step."""

    def __init__(self, dp, store=None):
        self.tier = is_gpu(dp) and bool(dp.info.get("spill_bytes"))
        self.store = store
        self.ring = RingModel()
        self.moved = []
        self.now = NOW
        self.notes = {}

    def last(self, kind):
        return [b for k, b in self.moved if k == kind]


def as_list(v):
    return [] if v is None else (v if isinstance(v, list) else [v])     # (an empty dict is one call with the defaults)


def apply_tier(dp, ctx, inp):
    sp, st, co, ci, fn = (inp.pop(k, None) for k in ("__spill__", "__stage_spill__", "__cold_out__", "__cold_in__",
                                                     "__tier__"))
    if not ctx.tier:
        return
    for kw in as_list(sp):
        if "lim" in kw:
            ctx.moved.append(("spill", int(dp.eng.spill(int(kw["lim"]), int(kw.get("hot", 0))))))
        else:
            ctx.moved.append(("spill", int(dp.spill(frac=kw.get("frac", 1.0), hot=kw.get("hot", 0)))))
    for kw in as_list(st):
        dp.eng.stage_spill(int(kw["frac"]), int(kw.get("hot", 0)), int(kw.get("budget", 0)))
    for kw in as_list(co):
        _, kept = cold_out(dp, ctx.store, **kw)
        ctx.moved.append(("cold_out", 0 if kept is None else int(kept["bytes"].sum())))
    for kw in as_list(ci):
        ctx.notes["before_cold_in"] = dict(ring=ring_state(dp), lim=dev(dp, "q_cold_lim"))   # what k_cold_scan will see
        ctx.moved.append(("cold_in", int(dp.cold_in(ctx.store, **kw))))
    if fn is not None:
        try:
            fn(dp, ctx)
        except AssertionError as e:
            raise AssertionError(f"{e}\n[tier operations so far: {ctx.moved}; live bytes {live_sums(dp)}]") from e


def run_tier(dp, steps, ctx, now_step_ms=STEP_MS):
    outs = []
    for k, inp in enumerate(steps):
        inp = dict(inp)
        do = inp.pop("__do__", None)
        if do is not None:
            do(dp)
        for op in inp.pop("__ops__", []):
            getattr(dp, op[0])(*op[1], **(op[2] if len(op) > 2 else {}))
        ctx.now = NOW + now_step_ms * k
        apply_tier(dp, ctx, inp)
        gets = serve_gets(dp, inp.pop("__get__", []), ctx.now)
        r = dp.step(inp, now_ms=ctx.now)
        o = step_out(dp, r, gets)
        if ctx.tier:
            o["spill_moved"] = int(r.counters.get("spill_moved", 0))
            ctx.ring.end_step()
        outs.append(o)
    return outs


def seen_by_conn(outs):
    """What each connection saw over the whole run, in its order."""
    by = {}
    for s in observe(outs):
        by.setdefault(s.conn, []).append((s.ch, s.kind, s.ctag, s.tag, s.redelivered, s.body, tuple(s.frames or ())))
    return by


def assert_end_state(dp, ctx, orphans=(0, 0, 0, 0)):
    """After everything is consumed and acked and SPILL_LAG + 1 empty steps: no live message, no
    live byte in any tier, the ring's tail within a block of its head, and the store's gc
    unlinks every segment but the current one.  ``orphans`` = (messages, log bytes, ring bytes,
    cold bytes) a scenario leaves behind on purpose."""
    for k in range(SPILL_LAG + 1):
        dp.step({}, now_ms=ctx.now + 1 + k)
    msgs, logb, ringb, coldb = orphans
    c = dp.last_counters
    assert (c["n_live_msgs"], c["live_bytes"]) == (msgs, logb), (c["n_live_msgs"], c["live_bytes"])
    sums = live_sums(dp)
    assert sums == dict(log=logb, spill=ringb, cold=coldb), sums
    if not any(orphans):   # every entry, not only the sums (a byte released twice is negative somewhere)
        assert not dp.cold_live().any() and not dev(dp, "spill_live", "<i8").any() and not dev(dp, "log_live", "<i8").any()
    assert dev1(dp, "spill_head") - dev1(dp, "spill_tail") < LOG_BLOCK
    if ctx.store is not None and not coldb:
        ctx.store.gc(dp.cold_live())
        assert set(ctx.store.fds) <= {ctx.store.head >> SEG_SHIFT}, "a released segment was not unlinked"


def attach(conn, q, tag, no_ack=True, ch=1):
    return ("consume", (conn, ch, VH, q, tag), dict(no_ack=no_ack))


ACK_ALL = ack_frame(1, 0, multiple=True)


def in_order(outs, conn, q, n, redelivered=False):
    """Connection ``conn`` got queue ``q``'s messages 0..n-1 once, in order, each body intact."""
    mine = [s for s in observe(outs) if s.conn == conn and s.kind == "deliver"]
    assert [serial(s.body) for s in mine] == [(q, i) for i in range(n)], [serial(s.body) for s in mine][:8]
    return mine


# ---------------------------------------------------------------- spill, content
CONTENT_SIZES = (10, 255, 256, FM - 9, FM - 8, FM - 7, 3 * (FM - 8) + 5, 4000, 16)


def content_body(i, n):
    return bytes((7 * i + k * (i + 1)) & 255 for k in range(n))


def sc_spill_content(dp, ctx):
    """Bodies of distinct content and mixed sizes -- shorter than ref_min (256), exactly one body
    frame of the consumer's connection (frame-max 4096), one byte more, several frames --
    spilled with spill(1.0, hot 0) and then delivered: by reference from the ring (the default)
    or inline (egress_ref None).  All of them moved, nothing is left in the log."""
    dp.declare_queue(VH, "sq")
    open_ch(dp, 1)
    open_ch(dp, 2, frame_max=FM)
    bodies = [content_body(i, n) for i, n in enumerate(CONTENT_SIZES)]
    total = sum(slot_of("sq", b) for b in bodies)

    def moved_all(dp, ctx):
        assert ctx.last("spill") == [total, 0]
        assert live_sums(dp) == dict(log=0, spill=total, cold=0)     # conservation, mixed sizes
    return [{1: b"".join(publish_command(1, "", "sq", b) for b in bodies)},
            {"__spill__": [dict(frac=1.0, hot=0), dict(frac=1.0, hot=0)], "__tier__": moved_all,
             "__ops__": [attach(2, "sq", "c")]}, {}]


def ck_spill_content(outs):
    mine = [s for s in observe(outs) if s.conn == 2]
    assert [s.body for s in mine] == [content_body(i, n) for i, n in enumerate(CONTENT_SIZES)]
    assert all(max(s.frames or [0]) <= FM - 8 for s in mine) and {s.step for s in mine} == {1}


# ---------------------------------------------------------------- spill, selection
POW = 8


def pow_body(q, i):
    """Message i has a slot of 64 << i bytes: a sum of slots names the set that moved."""
    return body_of(q, i, (64 << i) - 16)


def pow_slots(idx):
    return sum(64 << i for i in idx)


def sc_spill_hot(dp, ctx):
    """A consumer out of credit (prefetch 2, manual ack) holds entries 0 and 1; the head is 2.
    spill(hot 3) moves exactly the entries from position head + 3 = 5 on; the two unacked
    deliveries and the three hot entries stay in the log; a second spill moves nothing."""
    dp.declare_queue(VH, "hq")
    open_ch(dp, 1)
    open_ch(dp, 2)
    dp.qos(2, 1, prefetch_count=2)
    dp.consume(2, 1, VH, "hq", "c", no_ack=False)

    def expect(dp, ctx):
        assert ctx.last("spill") == [pow_slots(range(5, POW)), 0]
        assert live_sums(dp) == dict(log=pow_slots(range(5)), spill=pow_slots(range(5, POW)), cold=0)
    return [{1: b"".join(publish_command(1, "", "hq", pow_body("hq", i)) for i in range(POW))},
            {"__spill__": [dict(frac=1.0, hot=3)] * 2, "__tier__": expect, "__ops__": [("qos", (2, 1, 0))], 2: ACK_ALL},
            {2: ACK_ALL}, {}]


def ck_queue_in_order(q, n, conn=2):
    def ck(outs):
        in_order(outs, conn, q, n)
    return ck


def sc_spill_lim(dp, ctx):
    """No consumer: the move starts at the head.  eng.spill(lim) with lim at the start of entry
    5's slot moves exactly entries 0..4 (slot start below lim); one byte more takes entry 5."""
    dp.declare_queue(VH, "lq")
    open_ch(dp, 1)
    open_ch(dp, 2)
    lim = pow_slots(range(5))     # the log starts at 0: slot i starts at the sum of the slots before it

    def expect(dp, ctx):
        assert dev1(dp, "log_head") == pow_slots(range(POW))
        assert ctx.last("spill") == [pow_slots(range(5)), pow_slots([5]), pow_slots([6, 7]), 0]
    return [{1: b"".join(publish_command(1, "", "lq", pow_body("lq", i)) for i in range(POW))},
            {"__spill__": [dict(lim=lim), dict(lim=lim + 1), dict(frac=1.0), dict(frac=1.0)], "__tier__": expect,
             "__ops__": [attach(2, "lq", "c")]}, {}]


def sc_spill_fanout(dp, ctx):
    """A message fanned out to two queues moves once: the moved bytes count it once, both queues
    deliver it intact, and it is released once (the end state holds no negative byte)."""
    dp.declare_exchange(VH, "fx", "fanout")
    for q in ("fa", "fb"):
        dp.declare_queue(VH, q)
        dp.bind(VH, q, "fx", "")
    open_ch(dp, 1)
    open_ch(dp, 2)
    open_ch(dp, 3)
    bodies = [body_of("fx", i, 500 + 16 * i) for i in range(3)]
    total = sum(slot_of("k", b, ex="fx") for b in bodies)

    def expect(dp, ctx):
        assert ctx.last("spill") == [total, 0]
        assert live_sums(dp) == dict(log=0, spill=total, cold=0)
    return [{1: b"".join(publish_command(1, "fx", "k", b) for b in bodies)},
            {"__spill__": [dict(frac=1.0)] * 2, "__tier__": expect, "__ops__": [attach(2, "fa", "a"), attach(3, "fb", "b")]},
            {}]


def ck_spill_fanout(outs):
    in_order(outs, 2, "fx", 3)
    in_order(outs, 3, "fx", 3)


CUR_SIZE = 1008      # slot 1024


def sc_spill_cursor(dp, ctx):
    """The cursor (q_spill_cur).  Entries 0..2 are delivered unacked (not moved: the spill takes
    3..5, a second one nothing); they are nack-requeued in front of the cursor and the next
    spill moves exactly them; the consumer then takes everything and three more, so the head
    passes the cursor, and a spill of three new entries still finds them."""
    S = slot_of("cq", body_of("cq", 0, CUR_SIZE))
    dp.declare_queue(VH, "cq")
    open_ch(dp, 1)
    open_ch(dp, 2)
    dp.qos(2, 1, prefetch_count=3)
    dp.consume(2, 1, VH, "cq", "c", no_ack=False)

    def expect(want):
        def fn(dp, ctx):
            assert ctx.last("spill") == want, (ctx.last("spill"), want)
        return fn
    return [{1: pubs("cq", 0, 6, CUR_SIZE)},
            {"__spill__": [dict(frac=1.0)] * 2, "__tier__": expect([3 * S, 0]), "__ops__": [("flow", (2, 1, False))],
             2: nack(1, 0)},
            {"__spill__": dict(frac=1.0), "__tier__": expect([3 * S, 0, 3 * S]),
             "__ops__": [("flow", (2, 1, True)), ("qos", (2, 1, 0))]},
            {2: ACK_ALL, 1: pubs("cq", 6, 9, CUR_SIZE)},
            {"__ops__": [("flow", (2, 1, False))], 2: ACK_ALL, 1: pubs("cq", 9, 12, CUR_SIZE)},
            {"__spill__": [dict(frac=1.0)] * 2, "__tier__": expect([3 * S, 0, 3 * S, 3 * S, 0]),
             "__ops__": [("flow", (2, 1, True))]},
            {2: ACK_ALL}, {}]


def ck_spill_cursor(outs):
    mine = [s for s in observe(outs) if s.conn == 2]
    assert [(serial(s.body)[1], s.redelivered) for s in mine] == (
        [(i, False) for i in range(3)] + [(i, True) for i in range(3)] + [(i, False) for i in range(3, 12)])


# ---------------------------------------------------------------- spill inside the step
def sc_stage_spill(dp, ctx):
    """eng.stage_spill(frac, hot, budget): with equal slots of S bytes and a budget of 2.5 S a step
    moves exactly floor(B / S) = 2 slots (spill_moved says so) until nothing is left: five steps
    for ten entries, then 0.  Budget 0 is unlimited: ten more entries move in one step."""
    dp.declare_queue(VH, "bq")
    open_ch(dp, 1)
    open_ch(dp, 2)
    full = dict(frac=65536, hot=0)
    return ([{1: pubs("bq", 0, 10, B4K)}, {"__stage_spill__": dict(full, budget=int(2.5 * S4K))}] + [{}] * 5
            + [{"__stage_spill__": dict(frac=0), 1: pubs("bq", 10, 20, B4K)}, {"__stage_spill__": dict(full, budget=0)},
               {"__stage_spill__": dict(frac=0), "__ops__": [attach(2, "bq", "c")]}, {}])


STAGE_MOVED = [0] + [2 * S4K] * 5 + [0, 0, 10 * S4K, 0, 0]


def ck_stage_spill(outs):
    in_order(outs, 2, "bq", 20)
    if "spill_moved" in outs[0]:
        assert [o["spill_moved"] for o in outs] == STAGE_MOVED


# ---------------------------------------------------------------- ring wrap and reuse
WRAP_BODY = 4000
WRAP_S = 4016                      # does not divide the ring: 130 slots and 2208 bytes
WRAP_FIT = SPILL_BYTES // WRAP_S
WRAP_N, WRAP_MORE = 140, 20


def sc_ring_wrap(dp, ctx):
    """140 bodies whose slot (4016) does not divide the ring: the spill moves 130 slots and then
    reports 0 -- the 131st would be padded past the ring's end into bytes the tail has not
    left.  All are consumed in one step and acked in the next, which frees the ring up to the
    head's block; 20 more bodies wait with the channel's flow off.  spill() must not reuse the
    freed bytes before SPILL_LAG steps have recorded the new tail (it moves 0 after each of
    the next SPILL_LAG - 1 steps) and must after: the first new slot is padded to the wrap and
    lands at the ring's start.  Head, tail, lag and live bytes per block equal the replica."""
    assert slot_of("wq", body_of("wq", 0, WRAP_BODY)) == WRAP_S and WRAP_FIT == 130
    dp.declare_queue(VH, "wq")
    open_ch(dp, 1)
    open_ch(dp, 2)
    ring = ctx.ring

    def fill(dp, ctx):
        n = 0
        while ring.reserve(WRAP_S) is not None:
            n += 1
        assert n == WRAP_FIT and ctx.last("spill") == [WRAP_FIT * WRAP_S, 0]
        assert_ring(dp, ring)

    def acked(dp, ctx):     # the step that follows releases every slot of the first batch
        assert_ring(dp, ring)
        for p in range(WRAP_FIT):
            ring.release(p * WRAP_S, WRAP_S)

    def freed(dp, ctx):
        assert ring.tail == (ring.head // LOG_BLOCK) * LOG_BLOCK and ring.lagged_tail() == 0
        assert ctx.last("spill")[2:] == [0]
        assert_ring(dp, ring)

    def still_full(dp, ctx):
        assert ctx.last("spill")[-1] == 0, "freed ring bytes reused before SPILL_LAG steps recorded the tail"
        assert_ring(dp, ring)

    def reused(dp, ctx):
        first = ring.reserve(WRAP_S)
        assert first == SPILL_BYTES, "the first new slot is padded to the wrap"
        for _ in range(WRAP_MORE - 1):
            assert ring.reserve(WRAP_S) is not None
        assert ctx.last("spill")[-1] == WRAP_MORE * WRAP_S
        assert_ring(dp, ring)
    steps = [{1: pubs("wq", 0, WRAP_N, WRAP_BODY)},
             {"__spill__": [dict(frac=1.0)] * 2, "__tier__": fill, "__ops__": [attach(2, "wq", "c", no_ack=False)]},
             {"__ops__": [("flow", (2, 1, False))], "__tier__": acked, 2: ACK_ALL,
              1: pubs("wq", WRAP_N, WRAP_N + WRAP_MORE, WRAP_BODY)},
             {"__spill__": dict(frac=1.0), "__tier__": freed}]
    steps += [{"__spill__": dict(frac=1.0), "__tier__": still_full} for _ in range(SPILL_LAG - 2)]
    steps += [{"__spill__": dict(frac=1.0), "__tier__": reused, "__ops__": [("flow", (2, 1, True))]}, {2: ACK_ALL}, {}]
    return steps


# ---------------------------------------------------------------- cold out, selection
SEL_HOT = 2


def sc_cold_select(dp, ctx):
    """k_cold_pick takes only spilled, single-queue, non-persistent entries at least ``hot`` behind
    the head of a queue with consumers, below spill_tail + lim_rel: of queue cq (consumer out of
    credit, head 1) exactly positions 3..9 -- not the persistent messages of durable dq, not the
    two-queue messages of fa / fb, not cq's 10..12 that are still in the log.  lim_rel in the
    middle of the picked positions takes exactly those below it.  max_n 3 and max_bytes 2.5
    slots cut the batch: repeated calls move the rest, each entry once."""
    dp.declare_queue(VH, "cq")
    dp.declare_queue(VH, "dq", durable=True)
    dp.declare_exchange(VH, "fx", "fanout")
    for q in ("fa", "fb"):
        dp.declare_queue(VH, q)
        dp.bind(VH, q, "fx", "")
    open_ch(dp, 1)
    for conn in (2, 3, 4, 5):
        open_ch(dp, conn)
    dp.qos(2, 1, prefetch_count=1)
    dp.consume(2, 1, VH, "cq", "c", no_ack=False)
    S = S4K
    first = (pubs("cq", 0, 10, B4K) + pubs("dq", 0, 2, B4K, {"delivery_mode": 2})
             + b"".join(publish_command(1, "fx", "k", body_of("fx", i, B4K)) for i in range(2)))

    def select(dp, ctx):
        assert ctx.last("spill") == [13 * S]
        cq = dp.queues[(VH, "cq")].slot
        want = list(range(1 + SEL_HOT, 10))
        recs, _ = cold_out(dp, ctx.store, hot=SEL_HOT, commit=False)
        assert sorted((int(r["q"]), int(r["qpos"])) for r in recs) == [(cq, p) for p in want]
        assert all(int(r["bytes"]) == S for r in recs)
        pos = sorted(int(r["pos"]) for r in recs)
        below, _ = cold_out(dp, ctx.store, hot=SEL_HOT, frac=(pos[3] - dev1(dp, "spill_tail")) / SPILL_BYTES, commit=False)
        assert sorted(int(r["pos"]) for r in below) == pos[:3]
        # max_n 3: three records, committed; the cursor stays at the first entry left out
        three, kept = cold_out(dp, ctx.store, hot=SEL_HOT, max_n=3)
        assert len(three) == 3 and len(kept) == 3
        done = {int(r["qpos"]) for r in kept}
        sizes = []
        for _ in range(4):     # max_bytes 2.5 slots: two a call, the cut records carry bytes 0
            recs, kept = cold_out(dp, ctx.store, hot=SEL_HOT, max_bytes=int(2.5 * S))
            got = set() if kept is None else {int(r["qpos"]) for r in kept}
            assert not got & done, "an entry moved twice"
            assert all(int(r["bytes"]) in (0, S) for r in recs) and len(recs) == len(want) - len(done)
            done |= got
            sizes.append(len(got))
        assert sizes == [2, 2, 0, 0] and done == set(want)
        assert cold_lim(dp, "cq") == 1 + SEL_HOT
        assert live_sums(dp) == dict(log=4 * S, spill=6 * S, cold=7 * S)     # cq 0 (unacked) and 10..12 in the log
        ctx.moved.append(("cold_in", int(dp.cold_in(ctx.store))))
        assert ctx.last("cold_in") == [7 * S] and cold_lim(dp, "cq") == NOT_HELD
    return [{1: first}, {"__spill__": dict(frac=1.0), 1: pubs("cq", 10, 13, B4K)},
            {"__tier__": select, "__ops__": [("qos", (2, 1, 0))], 2: ACK_ALL},     # (dq, fa, fb without consumers: no hot entries)
            {"__ops__": [attach(3, "dq", "d"), attach(4, "fa", "a"), attach(5, "fb", "b")], 2: ACK_ALL}, {}]


def ck_cold_select(outs):
    in_order(outs, 2, "cq", 13)
    in_order(outs, 3, "dq", 2)
    in_order(outs, 4, "fx", 2)
    in_order(outs, 5, "fx", 2)


# ---------------------------------------------------------------- commit races with a delivery
def sc_commit_race(dp, ctx):
    """cold_pick of eight spilled entries, then a step in which a consumer takes the first two,
    then cold_commit of the full batch: the two stay spilled (their ring bytes are released by
    the ack, once), six go cold, q_cold_lim is 2 and cold_live counts six slots."""
    dp.declare_queue(VH, "rq")
    open_ch(dp, 1)
    open_ch(dp, 2)
    S = S4K

    def pick(dp, ctx):
        assert ctx.last("spill") == [8 * S]
        recs, kept = cold_out(dp, ctx.store, commit=False)
        assert sorted(int(r["qpos"]) for r in kept) == list(range(8))
        ctx.notes["batch"] = kept

    def commit(dp, ctx):
        dp.eng.cold_commit(ctx.notes["batch"])
        assert cold_lim(dp, "rq") == 2
        assert live_sums(dp) == dict(log=0, spill=2 * S, cold=6 * S)
        ctx.moved.append(("cold_in", int(dp.cold_in(ctx.store))))
        assert ctx.last("cold_in") == [6 * S] and live_sums(dp) == dict(log=0, spill=8 * S, cold=0)
    return [{1: pubs("rq", 0, 8, B4K)},
            {"__spill__": dict(frac=1.0), "__tier__": pick,
             "__ops__": [("qos", (2, 1, 2)), attach(2, "rq", "c", no_ack=False)]},
            {"__tier__": commit, "__ops__": [("qos", (2, 1, 0))], 2: ACK_ALL}, {2: ACK_ALL}, {}]


# ---------------------------------------------------------------- the hold at the first cold position
HOLD_N, HOLD_P, HOLD_SIZE = 80, 10, 240


def sc_cold_hold(window):
    def sc(dp, ctx):
        dp.declare_queue(VH, "hq")
        open_ch(dp, 1)
        open_ch(dp, 2)
        rounds = -(-(HOLD_N - HOLD_P) // min(window, HOLD_N))
        S = slot_of("hq", body_of("hq", 0, HOLD_SIZE))

        def out(dp, ctx):
            assert ctx.last("spill") == [HOLD_N * S] and ctx.last("cold_out") == [(HOLD_N - HOLD_P) * S]
            assert cold_lim(dp, "hq") == HOLD_P
        steps = [{1: pubs("hq", 0, HOLD_N, HOLD_SIZE)},
                 {"__ops__": [attach(2, "hq", "c"), ("flow", (2, 1, False))], "__spill__": dict(frac=1.0),
                  "__cold_out__": dict(hot=HOLD_P), "__tier__": out},
                 {"__ops__": [("flow", (2, 1, True))]}, {}]
        steps += [{"__cold_in__": dict(window=window)} for _ in range(rounds)]
        return steps + [{}]
    sc.__doc__ = f"""Entries {HOLD_P}.. of {HOLD_N} are cold and the consumer has ample credit: a step delivers exactly
    positions 0..{HOLD_P - 1} and nothing further, the next step nothing; after each cold_in(window {window}) the next
    step delivers exactly the window's entries from the head, up to the scan's end."""
    return sc


def ck_cold_hold(window):
    def ck(outs):
        mine = in_order(outs, 2, "hq", HOLD_N)
        if "spill_moved" not in outs[0]:
            return            # (the golden run has no hold: the order and the bodies are all it shows)
        per = [sum(1 for s in mine if s.step == k) for k in range(len(outs))]
        want, left = [0, 0, HOLD_P, 0], HOLD_N - HOLD_P
        while left:
            want.append(min(window, left))
            left -= want[-1]
        assert per == want + [0], (per, want)
    return ck


# ---------------------------------------------------------------- cold in, room
ROOM_COLD, ROOM_OTHER = 64, 80


def room_rounds():
    return 2 * SPILL_LAG + 4


def sc_cold_in_room(dp, ctx):
    """64 consecutive cold entries of 4 KiB slots (256 KiB) while 80 spilled entries of another
    queue leave 192 KiB of the ring free: one wave's bodies exceed the free room.  cold_in pages
    in the longest prefix that fits -- 48 -- and q_cold_lim sits at the first entry left out;
    every call pages in at least the first cold entry while the ring has room for one slot, and
    repeated calls with steps in between drain the queue."""
    for q in ("cq", "oq"):
        dp.declare_queue(VH, q)
    open_ch(dp, 1)
    open_ch(dp, 2)
    open_ch(dp, 3)
    S = S4K

    def out(dp, ctx):
        assert ctx.last("spill") == [ROOM_COLD * S] and ctx.last("cold_out") == [ROOM_COLD * S]
        assert cold_lim(dp, "cq") == 0

    def fill(dp, ctx):
        assert ctx.last("spill")[-1] == ROOM_OTHER * S
        st = ring_state(dp)
        assert st["head"] - min([st["tail"]] + st["lag"]) == ROOM_OTHER * S     # the ring's free room: 48 slots
    steps = [{1: pubs("cq", 0, ROOM_COLD, B4K)}, {"__spill__": dict(frac=1.0), "__cold_out__": dict(), "__tier__": out}]
    steps += [{} for _ in range(SPILL_LAG)]                     # the ring's tail follows, and its lag
    steps += [{1: pubs("oq", 0, ROOM_OTHER, B4K)}, {"__spill__": dict(frac=1.0), "__tier__": fill},
              {"__cold_in__": dict(), "__tier__": both(paged_in("cq", S, (SPILL_BYTES - ROOM_OTHER * S) // S), progress("cq", S, ROOM_COLD)),
               "__ops__": [attach(2, "cq", "c"), attach(3, "oq", "o")]}]
    steps += [{"__cold_in__": dict(), "__tier__": progress("cq", S, ROOM_COLD)} for _ in range(room_rounds())]
    return steps + [{}]


def both(f, g):
    def fn(dp, ctx):
        f(dp, ctx)
        g(dp, ctx)
    return fn


def paged_in(q, S, n):
    def fn(dp, ctx):
        assert ctx.last("cold_in")[-1] == n * S, (ctx.last("cold_in"), n)
        assert cold_lim(dp, q) == n, "q_cold_lim is not at the first entry left out"
    return fn


def progress(q, S, total, exact=None):
    """After a cold_in of queue ``q`` (``total`` entries of slot S, all cold from q_cold_lim on), judged
    by the state read *before* the call: it paged in exactly the longest prefix of the cold entries
    that the ring had room for -- so at least the first one whenever one slot fitted -- and
    q_cold_lim sits at the first entry left out (~0 when none is)."""
    def fn(dp, ctx):
        moved = ctx.last("cold_in")[-1]
        before = ctx.notes["before_cold_in"]
        st, lim = before["ring"], int(before["lim"][dp.queues[(VH, q)].slot])
        left = 0 if lim == NOT_HELD else total - lim
        tail = min([st["tail"]] + st["lag"])
        fit = max([k for k in range(left + 1) if k == 0 or RingModel().fits(k * S, head=st["head"], tail=tail) is not None])
        assert moved == fit * S, (moved // S, fit, left, st)
        assert not (left and RingModel().fits(S, head=st["head"], tail=tail) is not None and moved == 0)
        if left:
            assert cold_lim(dp, q) == (NOT_HELD if fit == left else lim + fit)
        if exact is not None:
            assert fit == exact, (fit, exact)
    return fn


def ck_room(outs):
    in_order(outs, 2, "cq", ROOM_COLD)
    in_order(outs, 3, "oq", ROOM_OTHER)


BIG_BODY = 8400
BIG_S = 8416            # 64 of them are 538 624 bytes: more than the whole ring
BIG_FIT = SPILL_BYTES // BIG_S
BIG_FIRST = (SPILL_BYTES - 2 * BIG_S) // BIG_S       # the first page-in: what fits between the head and the wrap


def sc_cold_in_ring(dp, ctx):
    """64 consecutive cold entries whose slots together exceed spill_bytes itself (64 x 8416): no
    single reservation could ever hold the wave.  Every cold_in pages in the longest prefix that
    fits (never across the ring's wrap), and the queue drains over repeated calls."""
    assert slot_of("gq", body_of("gq", 0, BIG_BODY)) == BIG_S and 64 * BIG_S > SPILL_BYTES and BIG_FIT == 62
    dp.declare_queue(VH, "gq")
    open_ch(dp, 1)
    open_ch(dp, 2)

    def first(dp, ctx):
        assert ctx.last("spill") == [BIG_FIT * BIG_S] and ctx.last("cold_out") == [BIG_FIT * BIG_S]

    def second(dp, ctx):
        assert ctx.last("spill")[-1] == 2 * BIG_S and ctx.last("cold_out")[-1] == 2 * BIG_S
        assert cold_lim(dp, "gq") == 0 and live_sums(dp) == dict(log=0, spill=0, cold=64 * BIG_S)
    steps = [{1: pubs("gq", 0, 64, BIG_BODY)}, {"__spill__": dict(frac=1.0), "__cold_out__": dict(), "__tier__": first}]
    steps += [{} for _ in range(SPILL_LAG)]
    steps += [{"__spill__": dict(frac=1.0), "__cold_out__": dict(), "__tier__": second}]
    steps += [{} for _ in range(SPILL_LAG)]
    # the first call: the ring's head is 16 832 bytes into its second lap with the lagged tail at that lap's start, so 60
    # slots (504 960 bytes) fit in front of the wrap and 61 would have to be padded past it into live bytes
    steps += [{"__cold_in__": dict(), "__tier__": progress("gq", BIG_S, 64, exact=BIG_FIRST if k == 0 else None),
               "__ops__": [attach(2, "gq", "c")] if k == 0 else []} for k in range(room_rounds())]
    return steps + [{}]


def ck_ring(outs):
    in_order(outs, 2, "gq", 64)


# ---------------------------------------------------------------- cold entries that die
DIE_N, DIE_SIZE = 20, 240


def sc_cold_die(dp, ctx):
    """Cold entries that expire (queue tq) or are purged (queue pq), without a dead-letter exchange:
    cold_live and the message table are released with no page-in, and messages published
    afterwards are delivered by the next steps without any cold_in call."""
    for q in ("tq", "pq"):
        dp.declare_queue(VH, q)
    open_ch(dp, 1)
    open_ch(dp, 2)
    open_ch(dp, 3)
    S = slot_of("tq", body_of("tq", 0, DIE_SIZE), SHORT)
    S2 = slot_of("pq", body_of("pq", 0, DIE_SIZE))

    def out(dp, ctx):
        assert ctx.last("cold_out") == [DIE_N * (S + S2)]
        assert cold_lim(dp, "tq") == 0 and cold_lim(dp, "pq") == 0

    def purge(dp):
        assert dp.purge(dp.queues[(VH, "pq")].slot) == DIE_N

    def gone(dp, ctx):
        assert live_sums(dp) == dict(log=0, spill=0, cold=0) and dp.last_counters["n_live_msgs"] == 0
        assert not ctx.last("cold_in")
    return [{1: pubs("tq", 0, DIE_N, DIE_SIZE, SHORT) + pubs("pq", 0, DIE_N, DIE_SIZE)},
            {"__spill__": dict(frac=1.0), "__cold_out__": dict(), "__tier__": out, "__do__": purge},
            {"__tier__": gone, 1: pubs("tq", 100, 105, DIE_SIZE) + pubs("pq", 100, 105, DIE_SIZE),
             "__ops__": [attach(2, "tq", "t"), attach(3, "pq", "p")]},
            {1: pubs("tq", 105, 107, DIE_SIZE)}, {}]


def ck_cold_die(outs):
    seen = observe(outs)
    assert [(s.step, serial(s.body)) for s in seen if s.conn == 2] == (
        [(2, ("tq", i)) for i in range(100, 105)] + [(3, ("tq", i)) for i in (105, 106)])
    assert [(s.step, serial(s.body)) for s in seen if s.conn == 3] == [(2, ("pq", i)) for i in range(100, 105)]
    assert outs[1]["counters"]["n_expired"] == 2 * DIE_N


DLX_COLD_CFG = dict(dead_letter=True, dead_max=64, dead_bytes=1 << 20, queue_limits=True)
DLX_N, DLX_P = 12, 4


def sc_cold_die_dlx(dp, ctx):
    """With a dead-letter exchange the TTL walk (queue src) and the x-max-length trim (queue lim,
    limit 10) stop at q_cold_lim -- the dead pass could not copy a cold body -- and continue after
    cold_in: the dead letters carry the original bodies, in order."""
    dp.declare_exchange(VH, "dlx", "direct")
    for q in ("src", "lim"):      # a park queue and a connection per source: the hold shifts the two sources' dead
        dp.declare_queue(VH, "park-" + q)   # letters against each other, not the order of either
        dp.bind(VH, "park-" + q, "dlx", q)
    dp.declare_queue(VH, "src", dead_letter_exchange="dlx")
    dp.declare_queue(VH, "lim", dead_letter_exchange="dlx", max_length=10)
    for conn in (1, 2, 3, 4, 5):
        open_ch(dp, conn)
    for conn, q in ((2, "src"), (3, "lim")):
        dp.consume(conn, 1, VH, q, "c-" + q, no_ack=True)
        dp.flow(conn, 1, False)

    def out(dp, ctx):
        assert cold_lim(dp, "src") == DLX_P and cold_lim(dp, "lim") == DLX_P

    def held(dp, ctx):      # the walk and the trim took the resident heads and stopped at the cold ones
        depth = {q: dp.message_count(dp.queues[(VH, q)].slot) for q in ("src", "lim")}
        assert depth == dict(src=DLX_N - DLX_P, lim=10 + 5 - DLX_P), depth
        assert dp.last_counters["n_dl_expired"] == DLX_P and dp.last_counters["n_dl_maxlen"] == DLX_P
    return [{1: pubs("src", 0, DLX_N, DIE_SIZE, SHORT) + pubs("lim", 0, 10, DIE_SIZE)},
            {"__spill__": dict(frac=1.0), "__cold_out__": dict(hot=DLX_P), "__tier__": out, 1: pubs("lim", 10, 15, DIE_SIZE)},
            {"__tier__": held, "__cold_in__": dict(), "__ops__": [attach(4, "park-src", "ps"), attach(5, "park-lim", "pl")]},
            {"__ops__": [("flow", (3, 1, True))]}, {}]


def ck_cold_die_dlx(outs):
    seen = [s for s in observe(outs) if s.conn in (4, 5)]
    assert [serial(s.body) for s in seen if s.conn == 4] == [("src", i) for i in range(DLX_N)]
    assert [serial(s.body) for s in seen if s.conn == 5] == [("lim", i) for i in range(5)]
    assert all(len(s.body) == DIE_SIZE for s in seen)
    assert [serial(s.body) for s in observe(outs) if s.conn == 3] == [("lim", i) for i in range(5, 15)]
    assert outs[-1]["after"]["depth"] == {"park-src": 0, "park-lim": 0, "src": 0, "lim": 0}


# ---------------------------------------------------------------- a queue slot used again
REUSE_OLD, REUSE_P, REUSE_NEW = 30, 5, 12


def sc_slot_reuse(dp, ctx):
    """A queue that holds cold entries from position 5 on is deleted (the plane releases nothing:
    its 30 messages stay orphaned, a broker purges first) and a new queue lands on its slot: 12
    messages, more than the old hold position, are all delivered by one plain step."""
    dp.declare_queue(VH, "old")
    open_ch(dp, 1)
    open_ch(dp, 2)
    dp.consume(2, 1, VH, "old", "o", no_ack=True)
    dp.flow(2, 1, False)
    slot = dp.queues[(VH, "old")].slot
    S = slot_of("old", body_of("old", 0, DIE_SIZE))

    def out(dp, ctx):
        assert ctx.last("cold_out") == [(REUSE_OLD - REUSE_P) * S] and cold_lim(dp, "old") == REUSE_P

    def again(dp):
        dp.delete_queue(VH, "old")
        k = 0
        while len(dp.queues) < dp.q_max - 1:     # a freed slot is reused last
            dp.declare_queue(VH, f"fill{k}", capacity=16)
            k += 1
        dp.declare_queue(VH, "new")
        assert dp.queues[(VH, "new")].slot == slot
        dp.flow(2, 1, True)
        dp.consume(2, 1, VH, "new", "n", no_ack=True)
    return [{1: pubs("old", 0, REUSE_OLD, DIE_SIZE)},
            {"__spill__": dict(frac=1.0), "__cold_out__": dict(hot=REUSE_P), "__tier__": out},
            {"__do__": again, 1: pubs("new", 0, REUSE_NEW, DIE_SIZE)}, {}]


REUSE_ORPHANS = (REUSE_OLD, 0, REUSE_P * 256, (REUSE_OLD - REUSE_P) * 256)


def ck_slot_reuse(outs):
    mine = [s for s in observe(outs) if s.conn == 2]
    assert [(s.step, s.ctag, serial(s.body)) for s in mine] == [(2, "n", ("new", i)) for i in range(REUSE_NEW)]


# ---------------------------------------------------------------- segment accounting
SEG_N = 6


def sc_cold_segments(dp, ctx):
    """store.head preset 2.5 slots below a segment boundary: a batch of six straddles it, and
    cold_live[0] / cold_live[1] hold exactly the bytes of the records on each side; reading
    everything back brings both to 0 and gc unlinks the first segment."""
    dp.declare_queue(VH, "gq")
    open_ch(dp, 1)
    open_ch(dp, 2)
    S = S4K
    if ctx.store is not None:
        ctx.store.head = (1 << SEG_SHIFT) - int(2.5 * S)

    def out(dp, ctx):
        assert ctx.last("spill") == [SEG_N * S]
        recs, kept = cold_out(dp, ctx.store)
        seg = [int(c) >> SEG_SHIFT for c in kept["cold"]]
        assert sorted(seg) == [0, 0, 1, 1, 1, 1]
        live = dp.cold_live()
        assert (int(live[0]), int(live[1]), int(live.sum())) == (2 * S, 4 * S, SEG_N * S)
        assert sorted(ctx.store.fds) == [0, 1]
        assert dp.cold_in(ctx.store) == SEG_N * S and not dp.cold_live().any()
        assert ctx.store.gc(dp.cold_live()) == 1 and sorted(ctx.store.fds) == [1]
    return [{1: pubs("gq", 0, SEG_N, B4K)}, {"__spill__": dict(frac=1.0), "__tier__": out, "__ops__": [attach(2, "gq", "c")]},
            {}]


# ---------------------------------------------------------------- Basic.Get of a tiered head
def sc_get_tiered(dp, ctx):
    """Basic.Get of a head in the spill ring returns it intact; of a head in the cold store it
    answers (None, count) while the plane has no store attached -- the entry stays -- and pages
    it in through plane.cold_store once there is one."""
    dp.declare_queue(VH, "gq")
    open_ch(dp, 1)
    open_ch(dp, 2)
    S = slot_of("gq", body_of("gq", 0, 700))

    def cold(dp, ctx):
        assert ctx.last("cold_out") == [3 * S] and cold_lim(dp, "gq") == 1
        slot = dp.queues[(VH, "gq")].slot
        assert getattr(dp, "cold_store", None) is None
        assert dp.basic_get(2, 1, slot, True, now_ms=ctx.now) == (None, 3)
        assert dp.message_count(slot) == 3 and live_sums(dp)["cold"] == 3 * S
        dp.cold_store = ctx.store
    return [{1: pubs("gq", 0, 4, 700)}, {"__spill__": dict(frac=1.0), "__get__": [(2, 1, "gq", True)]},
            {"__cold_out__": dict(), "__tier__": cold, "__get__": [(2, 1, "gq", False), (2, 1, "gq", True)], 2: ACK_ALL},
            {"__get__": [(2, 1, "gq", True), (2, 1, "gq", True)]}, {}]


def ck_get_tiered(outs):
    got = [decode_get(a) for o in outs for a in o["gets"]]
    assert [(g.tag, g.count, g.body) for g in got[:4]] == [(i + 1, 3 - i, body_of("gq", i, 700)) for i in range(4)]
    assert got[4] is None


# ---------------------------------------------------------------- the tables
SCENARIOS, CHECKS, END = {}, {}, {}


def _add(name, fn, ck, cfg=None, lockstep=True, kw=None, orphans=(0, 0, 0, 0)):
    SCENARIOS[name] = Scenario(fn, dict(TIER, **(cfg or {})), STEP_MS, lockstep, kw or {})
    CHECKS[name] = ck
    END[name] = orphans


_add("spill_content_by_reference", sc_spill_content, ck_spill_content)
_add("spill_content_inline", sc_spill_content, ck_spill_content, kw=dict(egress_ref=None))
_add("spill_hot", sc_spill_hot, ck_queue_in_order("hq", POW))
_add("spill_lim", sc_spill_lim, ck_queue_in_order("lq", POW))
_add("spill_fanout", sc_spill_fanout, ck_spill_fanout)
_add("spill_cursor", sc_spill_cursor, ck_spill_cursor)
_add("stage_spill", sc_stage_spill, ck_stage_spill)
_add("ring_wrap", sc_ring_wrap, ck_queue_in_order("wq", WRAP_N + WRAP_MORE))
_add("cold_select", sc_cold_select, ck_cold_select)
_add("commit_race", sc_commit_race, ck_queue_in_order("rq", 8))
for _w in (1, 63, 64, 65, 1000):
    _add(f"cold_hold_w{_w}", sc_cold_hold(_w), ck_cold_hold(_w), lockstep=False)
_add("cold_in_room", sc_cold_in_room, ck_room, lockstep=False)
_add("cold_in_ring", sc_cold_in_ring, ck_ring, lockstep=False)
_add("cold_die", sc_cold_die, ck_cold_die)
_add("cold_die_dlx", sc_cold_die_dlx, ck_cold_die_dlx, cfg=DLX_COLD_CFG, lockstep=False)
_add("slot_reuse", sc_slot_reuse, ck_slot_reuse, orphans=REUSE_ORPHANS)
_add("cold_segments", sc_cold_segments, ck_queue_in_order("gq", SEG_N))
_add("get_tiered", sc_get_tiered, ck_get_tiered)
