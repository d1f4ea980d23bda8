"""The opt-in features of the GPU data plane, each described once.

Every layer reads ``TABLE``: ``utils/config.py`` (HOCON keys -> keywords), ``ControlState`` /
``GpuDataPlane`` / ``GoldenDataPlane`` (keywords -> attributes and the engine's cfg dict) and
``GpuBroker`` (its checks against the plane, its statistics).  A new feature is one row here, its
behaviour, and -- where a kernel has a variant for it -- one more argument to a ``with_flags``
call in ``csrc/kernels/engine.hip``.  All features are off by default; off, the argument or
method they serve is ignored as the reference ignores it, and the step launches what it
launched before.  No HIP and no torch in here.
"""

from dataclasses import dataclass, make_dataclass

ALWAYS, WHEN_ON = "always", "when on"   # how a flag reaches the engine's cfg dict (None: never)


@dataclass(frozen=True)
class Feature:
    name: str                  # the Python keyword, and the attribute of planes and brokers
    key: str                   # the HOCON key under chana.mq.gpu.
    doc: str
    requires: str = None       # the feature that has to be on as well
    single_rank: bool = False  # not served on a sharded plane / node
    engine: str = None         # ALWAYS: 0/1 in the engine's cfg; WHEN_ON: 1 there only when on
    # plane keywords read with the feature: (keyword, HOCON key, default or f(the ones before))
    params: tuple = ()
    # broker statistics: (statistic, the step counter it is fed from, gauge: assigned, not summed)
    stats: tuple = ()


TABLE = (
    Feature("headers_match", "headers-match",
            "Headers exchanges match on their bindings' arguments (the headers branch of route_one; "
            "off: they route as topic).  The plane does the matching; the broker passes Queue.Bind / "
            "Unbind and Exchange.Bind / Unbind arguments on only when it is on.  headers-bindings / "
            "headers-pairs (engine cfg hb_max / hp_max) bound the device's row table and pair pool.",
            params=(("hb_max", "headers-bindings", 1024), ("hp_max", "headers-pairs", lambda p: 4 * p["hb_max"]))),
    Feature("queue_limits", "queue-limits",
            "Queues honour Queue.Declare's x-max-length / x-overflow (q_limit: trim_head in k_dequeue, "
            "the refusal in enq_store; off: the device never reads the field).  The broker parses the "
            "arguments and passes them to the plane, which enforces them.",
            engine=ALWAYS,
            # trimmed from drop-head queues / refused by reject-publish queues
            stats=(("maxlen_dropped", "n_maxlen_dropped", False), ("maxlen_rejected", "n_maxlen_rejected", False))),
    Feature("queue_limit_bytes", "queue-limit-bytes",
            "Queues honour x-max-length-bytes under their x-overflow mode, which is the count limit's "
            "(q_blimit; the device keeps every queue's ready bytes in q_bytes: k_byte_room and the BL "
            "instantiations of k_ring_plan / k_enqueue / k_dequeue / k_basic_get; the step sorts its "
            "pairs on the materialised path at every key width).",
            requires="queue_limits", engine=WHEN_ON),
    Feature("priority_queues", "priority-queues",
            "Queues honour x-max-priority: a queue declared with P takes P + 1 consecutive slots, its "
            "lanes (q_prio / q_lane_base); k_prio_lane moves each routed pair to the lane of its "
            "publish's priority ahead of the sort, and k_prio_dispatch, behind the PRIO instantiation of "
            "k_dequeue, serves the base slot's consumers and Gets from the lanes in order.",
            single_rank=True, engine=WHEN_ON),
    Feature("dead_letter", "dead-letter",
            "Queues honour x-dead-letter-exchange / x-dead-letter-routing-key: entries that expire, are "
            "trimmed by x-max-length or are rejected without requeue join the device's dead list and "
            "are published to the exchange by the next step's dead pass (k_dead_pack; dead-max / "
            "dead-bytes bound the list and one pass's payload; off: the device never reads the fields).  "
            "Single rank: the exchange's queues may live on another rank, which the pass cannot reach yet.",
            single_rank=True, engine=ALWAYS,
            params=(("dead_max", "dead-max", 1024), ("dead_bytes", "dead-bytes", 8 << 20)),
            # dead-lettered by reason, dead letters lost, entries pending on the device's list
            stats=tuple(("dl_" + s, "n_dl_" + s, s == "pending")
                        for s in ("expired", "maxlen", "rejected", "unrouted", "dropped", "pending"))),
    Feature("x_death", "dead-letter-x-death",
            "The dead pass rewrites each dead letter's property bytes -- x-death / x-first-death-* "
            "headers, the expiration removed (k_dead_size, k_dead_pack<true>: dp_xdeath.h) -- and its "
            "routing refuses the queues the history bans (cycle detection; off: the bytes are verbatim "
            "and cycles go round).",
            requires="dead_letter", engine=ALWAYS,
            # (dead letter, queue) pairs refused: the queue is in the dead letter's own history
            stats=(("dl_cycle", "n_dl_cycle", False),)),
    Feature("alternate_exchange", "alternate-exchange",
            "Exchange.Declare's alternate-exchange argument is validated, kept and routed by: an exchange "
            "the walk of route_one matched without any destination hands the publish to the exchange it "
            "names (route_closure has the rule; x_alt; the ALT instantiations of k_route / k_import_route).",
            engine=ALWAYS,
            # (publish, exchange) pairs whose alternate exchange was taken
            stats=(("alt_routed", "n_alt", False),)),
)


class _Features:
    @classmethod
    def take(cls, kw):
        """The features named in the keyword dict ``kw``, popped out of it."""
        return cls(**{f.name: bool(kw.pop(f.name, False)) for f in TABLE})

    def asdict(self):
        return {f.name: getattr(self, f.name) for f in TABLE}

    def on(self):
        """The rows of the features that are on, in the table's order."""
        return [f for f in TABLE if getattr(self, f.name)]

    def validate(self, world=1):
        for f in self.on():
            if f.requires and not getattr(self, f.requires):
                raise ValueError(f"{f.name}=True needs {f.requires}=True")
            if f.single_rank and world > 1:
                raise ValueError(f"{f.name}=True is not served on a sharded plane (world > 1)")
        return self

    def engine_cfg(self):
        """What the engine's cfg dict holds of the flags (sub-parameters ride the plane's **cfg)."""
        return {f.name: int(getattr(self, f.name)) for f in TABLE
                if f.engine == ALWAYS or (f.engine == WHEN_ON and getattr(self, f.name))}

    @classmethod
    def from_config(cls, g, k="chana.mq.gpu."):
        """``g`` = Config.get -> (the features, the plane keywords of the ones that are on)."""
        self = cls(**{f.name: bool(g(k + f.key, False)) for f in TABLE})
        plane = {}
        for f in self.on():
            if f.requires and not getattr(self, f.requires):
                raise ValueError(f"{k}{f.key} needs {k}{BY_NAME[f.requires].key}")
            plane[f.name] = True
            for name, key, dflt in f.params:
                plane[name] = int(g(k + key, dflt(plane) if callable(dflt) else dflt))
        return self, plane


BY_NAME = {f.name: f for f in TABLE}
Features = make_dataclass("Features", [(f.name, bool, False) for f in TABLE], bases=(_Features,), frozen=True)
Features.__module__ = __name__
