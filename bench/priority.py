#!/usr/bin/env python3
"""What priority queues cost a step: 16 queues, each filled with 4000 publishes in four steps (16
connections x 1000 a step, 16-byte bodies, default exchange, priorities 0..3 in turn), then drained by one
no-ack consumer a queue.

  --mode prio     the queues are declared with x-max-priority 3: 4 lanes x 1000 entries each, drained
                  by k_prio_dispatch (behind k_dequeue<.., PRIO>, which only walks the lanes)
  --mode plain    ordinary queues of 4000 entries on the same plane, drained by k_dequeue
  --mode idle     no priority queue and no traffic: what the two launches a step adds (k_prio_lane,
                  k_prio_dispatch) cost on a plane that has nothing for them

  --prio 1        the plane is built with priority_queues
  --prio 0        the same plane with the flag off (the argument is ignored: plain FIFO queues)

Run it alone under ``rocprofv3 --kernel-trace --stats -- python bench/priority.py ...`` and read the
per-launch averages of k_prio_lane, k_prio_dispatch and k_dequeue; the script itself prints one JSON
line with the host clock's median step time of the drain (or idle) steps and the counters it saw."""

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

QUEUES, FILL, BODY, P = 16, 4000, 16, 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("prio", "plain", "idle"), default="prio")
    ap.add_argument("--prio", type=int, default=1)
    ap.add_argument("--steps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    from chanamq_amd.engine.dataplane import GpuDataPlane
    from chanamq_amd.engine.traffic import publish_command
    cap = 1 << 13
    dp = GpuDataPlane(c_max=64, chpc=4, q_max=128, x_max=16, cons_max=64, seg_max=64, cmd_max=1 << 17, pair_max=1 << 17,
                      deliv_max=1 << 17, msg_max=1 << 20, ucap=1 << 13, deliver_cap=1 << 13, ingress_cap=32 << 20,
                      egress_cap=64 << 20, log_bytes=256 << 20, log_block=1 << 20, ring_pool=128 * cap, tb_max=16,
                      carry_cap=1 << 16, dhash=256, req_max=256, default_queue_capacity=cap,
                      **({"priority_queues": True} if a.prio else {}))
    vh = "AMQ.DEFAULT"
    fill = {}
    if a.mode != "idle":
        for i in range(QUEUES):
            q = f"pq{i}"
            dp.declare_queue(vh, q, **({"max_priority": P} if a.mode == "prio" else {}))
            dp.open_connection(i, vh)
            dp.open_channel(i, 1)
            fill[i] = b"".join(publish_command(1, "", q, b"%016d" % k, {"priority": k % (P + 1)}) for k in range(FILL // 4))
    times, deliv = [], 0
    rounds = 1 if a.mode == "idle" else a.steps
    for rnd in range(rounds):
        if a.mode == "idle":
            for k in range(a.warmup + a.steps):
                t0 = time.perf_counter()
                dp.step({})
                if k >= a.warmup:
                    times.append(time.perf_counter() - t0)
            break
        # fill (no consumer yet), then one drain step with a consumer a queue, then detach them
        for _ in range(4):   # (a quarter a step: a connection's step input stays within its carry)
            r = dp.step(fill)
            assert r.counters["n_ring_full"] == 0 and r.counters["n_dropped_nomem"] == 0, r.counters
        for i in range(QUEUES):
            dp.consume(i, 1, vh, f"pq{i}", f"c{i}", no_ack=True)
        t0 = time.perf_counter()
        r = dp.step({})
        dt = time.perf_counter() - t0
        if rnd >= min(a.warmup, rounds - 1):
            times.append(dt)
        deliv += int(r.counters["n_deliv"])
        assert r.counters["n_deliv"] == QUEUES * FILL, r.counters
        for i in range(QUEUES):
            dp.cancel(i, 1, f"c{i}")
        dp.step({})   # (the no-ack deliveries leave the channels' windows)
    depth = [dp.message_count(q.slot) for q in dp.queues.values()] or [0]
    print(json.dumps(dict(mode=a.mode, prio=a.prio, steps=len(times), step_ms_median=round(statistics.median(times) * 1e3, 4),
                          delivered=deliv, depth_max=max(depth), priority_queues=int(dp.info["priority_queues"]))))


if __name__ == "__main__":
    main()
