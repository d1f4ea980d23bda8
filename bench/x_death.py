#!/usr/bin/env python3
"""What the x-death rewrite costs a step with a full dead list: bench/dead_letter.py's `dying`
workload (16 queues with a dead-letter exchange and no consumers, a parking queue behind a fanout
exchange, 16 connections publishing 64 messages each per step with a 1 ms expiration, so every
step `dead_max` = 1024 entries die and the 1024 of the step before are rendered), with x_death on
and off on the same tree.

  --history 0    messages without history (the rewrite creates the table and one element)
  --history 32   messages that arrive with a 32-element x-death array naming 32 declared (unbound)
                 queues: the rewrite walks it, puts a 33rd element in front, resolves 33 names, and
                 the routing checks each candidate queue against a ban row of 33 slots
  --x-death 0|1  the flag

Without arguments the four combinations run one after the other, each in a child process of its
own under a time limit (``--limit`` seconds); the first that fails or runs out of time ends the
run, and nothing is tried twice.  Each prints one JSON line with the host clock's median step
period and the counters it saw; the rewrite's cost per item is the difference of the two periods
of one history, divided by 1024."""

import argparse
import json
import signal
import statistics
import subprocess
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

QUEUES, PER_Q, NOW = 16, 64, 1_800_000_000_000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--history", type=int, choices=(0, 32), default=None)
    ap.add_argument("--x-death", type=int, choices=(0, 1), default=1)
    ap.add_argument("--steps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--limit", type=int, default=90, help="seconds one run may take")
    a = ap.parse_args()
    if a.history is None:
        for hist, xd in ((0, 0), (0, 1), (32, 0), (32, 1)):
            cmd = [sys.executable, __file__, "--history", str(hist), "--x-death", str(xd), "--steps", str(a.steps),
                   "--warmup", str(a.warmup), "--limit", str(a.limit)]
            try:
                rc = subprocess.run(cmd, timeout=a.limit + 15).returncode
            except subprocess.TimeoutExpired:
                rc = 124
            if rc:
                sys.exit(f"x_death bench: history {hist} x_death {xd} ended with status {rc}; the later runs were not made")
        return
    signal.alarm(a.limit)   # a step that hangs ends this process: SIGALRM's default action
    from chanamq_amd.engine.dataplane import GpuDataPlane
    from chanamq_amd.engine.traffic import publish_command
    from chanamq_amd.protocol.codec import Typed
    cap = 1 << 17
    dp = GpuDataPlane(c_max=64, chpc=4, q_max=64, x_max=16, cons_max=64, seg_max=64, cmd_max=1 << 15, pair_max=1 << 16,
                      deliv_max=4096, msg_max=1 << 20, ucap=256, ingress_cap=16 << 20, egress_cap=8 << 20,
                      log_bytes=1 << 30, log_block=1 << 20, ring_pool=(QUEUES + 1) * cap + 32 * 1024, tb_max=16, carry_cap=1 << 16,
                      dhash=256, req_max=256, default_queue_capacity=cap, restore_max=1024,
                      dead_letter=True, dead_max=1024, dead_bytes=8 << 20, **({"x_death": True} if a.x_death else {}))
    vh = "AMQ.DEFAULT"
    dp.declare_exchange(vh, "dlx", "fanout")
    dp.declare_queue(vh, "park")
    dp.bind(vh, "park", "dlx", "")
    props = {"expiration": "1"}
    if a.history:
        for i in range(a.history):   # the history's queues exist (so their names resolve) but are bound nowhere
            dp.declare_queue(vh, f"earlier{i}", capacity=1024)
        props["headers"] = {"x-death": [{"count": Typed("l", 1), "reason": "expired", "queue": f"earlier{i}",
                                         "time": Typed("T", 1_700_000_000 + i), "exchange": "",
                                         "routing-keys": [f"earlier{i}"]} for i in range(a.history)]}
    inputs = {}
    for i in range(QUEUES):
        q = f"dq{i}"
        dp.declare_queue(vh, q, dead_letter_exchange="dlx")
        dp.open_connection(i, vh)
        dp.open_channel(i, 1)
        inputs[i] = b"".join(publish_command(1, "", q, b"%016d" % k, props) for k in range(PER_Q))
    times, seen = [], dict.fromkeys(("n_expired", "n_dl_expired", "n_dl_unrouted", "n_dl_dropped", "n_dl_cycle"), 0)
    for k in range(a.warmup + a.steps):
        t0 = time.perf_counter()
        r = dp.step(inputs, now_ms=NOW + 10 * k)
        if k >= a.warmup:
            times.append(time.perf_counter() - t0)
        for c in seen:
            seen[c] += int(r.counters.get(c, 0))
        assert r.counters["n_ring_full"] == 0 and r.counters["n_dropped_nomem"] == 0, r.counters
    print(json.dumps(dict(history=a.history, x_death=a.x_death, steps=a.steps,
                          step_ms_median=round(statistics.median(times) * 1e3, 4),
                          parked=int(dp.message_count(dp.queues[(vh, "park")].slot)),
                          pending=int(r.counters.get("n_dl_pending", 0)), **seen)))


if __name__ == "__main__":
    main()
