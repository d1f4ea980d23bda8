"""Control operations staged while steps run (``GpuDataPlane.defer``, the broker's light
sections) in the ``consumer_scenarios`` style.  A scenario is ``(dp) -> steps``: it sets the
plane up synchronously and returns the steps; a step may carry

``__light__``    a list of sections, each a list of ``(control method, args[, kwargs])``: every
                 section runs inside ``light(dp)`` before the step is submitted;
``__reserve__``  ring entries taken with ``reserve_ring_chunk`` outside the sections (as the
                 broker's full lock does) for queues declared inside them;
``__golden__``   the sections the golden model applies before this step where that is not
                 ``__light__`` (two sections writing the same row ride two steps).

The golden model runs the same steps with one documented shift: a ``consume`` staged before
step k is applied to the golden plane after step k.  That is ``cons_active = 2`` on the device:
the consumer's rows land in step k, k_post makes it active, and it takes deliveries from step
k + 1 on (behind its Basic.ConsumeOk).  A ``cancel`` of a consumer still held back that way takes
the held consume with it.  Every other op applies before step k, as on the device.  The shift is
exact as long as the staged consumer is alone on its queue (the round-robin walk of a shared
queue counts the not-yet-active consumer; ``sc_third_consumer`` is judged by client-side
statements for that reason)."""

from contextlib import contextmanager

from chanamq_amd.engine.traffic import ack_frame, publish_command
from consumer_scenarios import COUNTERS, body_of, open_ch
from dp_scenarios import NOW, VH


@contextmanager
def light(dp):
    """What the broker's ``_LightLock`` does to the plane: one staged batch per section, table
    writes deferred inside it.  A no-op on the golden plane."""
    eng = getattr(dp, "eng", None)
    if eng is None:
        yield
        return
    eng.stage_begin()
    dp.defer = True
    try:
        yield
    finally:
        dp.defer = False
        eng.stage_end()


def pub(q, lo, hi, size=32, ex="", rk=None, ch=1):
    """Messages lo..hi-1 of queue ``q`` (bodies name the queue and their serial)."""
    return b"".join(publish_command(ch, ex, q if rk is None else rk, body_of(q, i, size)) for i in range(lo, hi))


ACK_ALL = ack_frame(1, 0, multiple=True)


# ---------------------------------------------------------------- runner
class Shift:
    """The golden side of the consume shift: consumes held back until their step has run."""

    def __init__(self, dp):
        self.dp, self.held = dp, []

    def apply(self, sections):
        for ops in sections:
            for op in ops:
                if op[0] == "consume":
                    self.held.append(op)
                    continue
                if op[0] == "cancel":
                    conn, ch, tag = op[1]
                    mine = [h for h in self.held if (h[1][0], h[1][1], h[1][4]) == (conn, ch, tag)]
                    if mine:
                        self.held.remove(mine[0])
                        continue
                call(self.dp, op)

    def after_step(self):
        for op in self.held:
            call(self.dp, op)
        self.held = []


def call(dp, op):
    return getattr(dp, op[0])(*op[1], **(op[2] if len(op) > 2 else {}))


def stage_sections(dp, sections):
    """The device side: each section one closed batch, nothing read from the device."""
    for ops in sections:
        with light(dp):
            for op in ops:
                call(dp, op)


def run_deferred(dp, steps, now_step_ms=3000):
    """``consumer_scenarios.run_consumer`` with every step's control ops staged in light
    sections.  The outputs carry ``pending``: ``deltas_pending()`` after the step (None on the
    golden plane)."""
    gpu = hasattr(dp, "eng")
    shift = None if gpu else Shift(dp)
    outs = []
    for k, inp in enumerate(steps):
        inp = dict(inp)
        sections = inp.pop("__light__", [])
        golden = inp.pop("__golden__", sections)
        reserve = inp.pop("__reserve__", 0)
        if gpu:
            if reserve:
                dp.reserve_ring_chunk(reserve)
            stage_sections(dp, sections)
        else:
            shift.apply(golden)
        r = dp.step(inp, now_ms=NOW + now_step_ms * k)
        if gpu:
            eg, ctrl, ev, segs, tx, cnt = r.egress, r.ctrl, r.events, [s[:4] for s in r.segs], r.txbuf, r.counters
        else:
            eg, ctrl, ev, segs, tx, cnt = r["egress"], r["ctrl"], r["events"], r["segs"], r.get("txbuf", []), r["counters"]
            shift.after_step()
        outs.append(dict(egress=eg, ctrl=sorted(ctrl), events=sorted(ev), gets=[], txbuf=sorted(tx),
                         segs=sorted((s[0], s[1], s[2], s[3]) for s in segs),
                         counters={c: int(cnt.get(c, 0)) for c in COUNTERS},
                         pending=dp.deltas_pending() if gpu else None))
    return outs


# ---------------------------------------------------------------- scenarios
def consume_op(conn, ch, q, tag, no_ack=True):
    return ("consume", (conn, ch, VH, q, tag), dict(no_ack=no_ack))


def sc_consume_handover(dp):
    """A backlog of 6; connection, channel and consumer staged before step 1, which also brings
    two more messages: step 1 delivers nothing, step 2 the eight from the head, in order."""
    dp.declare_queue(VH, "hq")
    open_ch(dp, 1)
    attach = [("open_connection", (2, VH)), ("open_channel", (2, 1)), consume_op(2, 1, "hq", "h")]
    return [{1: pub("hq", 0, 6)}, {1: pub("hq", 6, 8), "__light__": [attach]}, {}, {1: pub("hq", 8, 10)}, {}]


def sc_consume_cancel(dp):
    """Consume and cancel of one tag in one section: never a delivery.  Then a consume staged
    before step 3 and its cancel before step 4: the consumer would take deliveries from step 4
    on, and the cancel's step is step 4: none either.  A last consumer shows the queue intact."""
    dp.declare_queue(VH, "cq")
    open_ch(dp, 1)
    open_ch(dp, 2)
    return [{1: pub("cq", 0, 4)},
            {1: pub("cq", 4, 6), "__light__": [[consume_op(2, 1, "cq", "x"), ("cancel", (2, 1, "x"))]]},
            {1: pub("cq", 6, 8)},
            {1: pub("cq", 8, 10), "__light__": [[consume_op(2, 1, "cq", "y")]]},
            {1: pub("cq", 10, 12), "__light__": [[("cancel", (2, 1, "y"))]]},
            {"__light__": [[consume_op(2, 1, "cq", "z")]]}, {}, {}]


def sc_flow(dp):
    """Flow off staged before step 1, on before step 2: step 1 delivers nothing, step 2 both
    steps' messages, and no later step stops."""
    dp.declare_queue(VH, "fq")
    open_ch(dp, 1)
    open_ch(dp, 2)
    dp.consume(2, 1, VH, "fq", "f", no_ack=True)
    return [{1: pub("fq", 0, 4)},
            {1: pub("fq", 4, 8), "__light__": [[("flow", (2, 1, False))]]},
            {1: pub("fq", 8, 10), "__light__": [[("flow", (2, 1, True))]]},
            {1: pub("fq", 10, 12)}, {}]


def sc_qos(dp):
    """A manual-ack consumer holding 3 without a prefetch limit; prefetch 5 staged before step 1:
    of that step's six only two go out.  Prefetch 2 staged before step 3, after an ack of all."""
    dp.declare_queue(VH, "pq")
    open_ch(dp, 1)
    open_ch(dp, 2)
    dp.consume(2, 1, VH, "pq", "p", no_ack=False)
    return [{1: pub("pq", 0, 3)},
            {1: pub("pq", 3, 9), "__light__": [[("qos", (2, 1, 5))]]},
            {2: ACK_ALL},
            {2: ACK_ALL, "__light__": [[("qos", (2, 1, 2))]]},
            {1: pub("pq", 9, 12)}, {2: ACK_ALL}, {2: ACK_ALL}, {}]


def sc_channel_close(dp):
    """Two manual-ack consumers share six messages; Channel.Close of the first staged before
    step 1: its three are requeued in that step and go to the other with the flag; nothing is
    delivered on the closed channel afterwards."""
    dp.declare_queue(VH, "xq")
    open_ch(dp, 1)
    open_ch(dp, 2)
    open_ch(dp, 3)
    dp.consume(2, 1, VH, "xq", "a", no_ack=False)
    dp.consume(3, 1, VH, "xq", "b", no_ack=False)
    return [{1: pub("xq", 0, 6)},
            {"__light__": [[("close_channel", (2, 1))]]},
            {1: pub("xq", 6, 10)}, {3: ACK_ALL}, {}]


def sc_connection_close(dp):
    """Connection 2 holds unacked deliveries on two channels, connection 3 on one;
    Connection.Close of 2 staged before step 1: both channels' deliveries are requeued."""
    dp.declare_queue(VH, "kq")
    open_ch(dp, 1)
    open_ch(dp, 2, 1, 2)
    open_ch(dp, 3)
    dp.consume(2, 1, VH, "kq", "a1", no_ack=False)
    dp.consume(2, 2, VH, "kq", "a2", no_ack=False)
    dp.consume(3, 1, VH, "kq", "b", no_ack=False)
    return [{1: pub("kq", 0, 6)},
            {"__light__": [[("close_connection", (2,))]]},
            {1: pub("kq", 6, 8)}, {3: ACK_ALL}, {}]


def sc_confirm_select(dp):
    """Confirm.Select staged before step 1: that step's publishes are confirmed, step 0's not."""
    dp.declare_queue(VH, "nq")
    open_ch(dp, 1)
    open_ch(dp, 2)
    dp.consume(2, 1, VH, "nq", "n", no_ack=True)
    return [{1: pub("nq", 0, 2)},
            {1: pub("nq", 2, 5), "__light__": [[("confirm_select", (1, 1))]]},
            {1: pub("nq", 5, 6)}, {}]


def sc_topology(dp):
    """The light topology methods: an exchange declare and a bind staged before step 1, whose
    publishes route by them; the unbind before step 2, whose publishes no longer do; a new queue
    (its ring from the reserved chunk) before step 3, whose publish lands in it -- a consumer
    staged before step 4 gets it in step 5."""
    dp.declare_queue(VH, "ta")
    open_ch(dp, 1)
    open_ch(dp, 2)
    dp.consume(2, 1, VH, "ta", "t", no_ack=True)
    cap = dp.default_queue_capacity
    return [{1: pub("ta", 0, 2)},
            {1: pub("ta", 2, 5, ex="tx", rk="k1"),
             "__light__": [[("declare_exchange", (VH, "tx", "direct")), ("bind", (VH, "ta", "tx", "k1"))]]},
            {1: pub("ta", 5, 7, ex="tx", rk="k1") + pub("ta", 7, 8), "__light__": [[("unbind", (VH, "ta", "tx", "k1"))]]},
            {1: pub("tn", 0, 3), "__reserve__": 2 * cap, "__light__": [[("declare_queue", (VH, "tn"))]]},
            {"__light__": [[consume_op(2, 1, "tn", "new")]]},
            {1: pub("tn", 3, 4)}, {}]


def sc_two_sections_one_step(dp):
    """Two closed sections writing disjoint rows (two channels' rows) staged back to back
    before step 1: both ride it (``pending`` empty after it; the runner records that)."""
    dp.declare_queue(VH, "wa")
    dp.declare_queue(VH, "wb")
    open_ch(dp, 1)
    open_ch(dp, 2)
    open_ch(dp, 3)
    dp.consume(2, 1, VH, "wa", "a", no_ack=False)
    dp.consume(3, 1, VH, "wb", "b", no_ack=True)
    return [{1: pub("wa", 0, 2) + pub("wb", 0, 2)},
            {1: pub("wa", 2, 8) + pub("wb", 2, 4),
             "__light__": [[("qos", (2, 1, 3))], [("flow", (3, 1, False))]]},
            {2: ACK_ALL}, {"__light__": [[("flow", (3, 1, True))]]}, {}]


def sc_same_row_twice(dp):
    """Prefetch 1, then prefetch 5 on one channel, two sections staged before step 1: they write
    the same row, so the second rides step 2 -- as the golden model with one op per step.  The
    consumer (prefetch 2 so far, holding 2 of 10) acks everything each step: one delivery in
    step 1, five in step 2, the last two in step 3."""
    dp.declare_queue(VH, "rq")
    open_ch(dp, 1)
    open_ch(dp, 2)
    dp.qos(2, 1, 2)
    dp.consume(2, 1, VH, "rq", "r", no_ack=False)
    one, five = [("qos", (2, 1, 1))], [("qos", (2, 1, 5))]
    return [{1: pub("rq", 0, 10)},
            {2: ACK_ALL, "__light__": [one, five], "__golden__": [one]},
            {2: ACK_ALL, "__golden__": [five]},
            {2: ACK_ALL}, {2: ACK_ALL}, {}]


def sc_third_consumer(dp):
    """Three auto-ack consumers on one queue: two present, the third staged before step 1, six
    messages a step.  Judged by client-side statements only (``ck_third_consumer``)."""
    dp.declare_queue(VH, "mq")
    open_ch(dp, 1)
    for conn, tag in ((2, "a"), (3, "b")):
        open_ch(dp, conn)
        dp.consume(conn, 1, VH, "mq", tag, no_ack=True)
    open_ch(dp, 4)
    return [{1: pub("mq", 0, 6)},
            {1: pub("mq", 6, 12), "__light__": [[consume_op(4, 1, "mq", "c")]]},
            {1: pub("mq", 12, 18)}, {1: pub("mq", 18, 24)}, {}]


SCENARIOS = {
    "consume_handover": sc_consume_handover,
    "consume_cancel": sc_consume_cancel,
    "flow": sc_flow,
    "qos": sc_qos,
    "channel_close": sc_channel_close,
    "connection_close": sc_connection_close,
    "confirm_select": sc_confirm_select,
    "topology": sc_topology,
    "two_sections_one_step": sc_two_sections_one_step,
    "same_row_twice": sc_same_row_twice,
}
assert all(len(fn.__doc__) > 0 for fn in SCENARIOS.values())
