#!/usr/bin/env python3
"""What a drop-head trim costs in k_dequeue: 16 queues without consumers, each taking 1000
publishes a step (16 connections x 1000, 16-byte bodies, default exchange).

  --limits 1   the queues are declared with x-max-length = 1024: from the second step on every
               queue trims about 1000 entries at the end of each step
  --limits 0   the same plane and traffic with the option off: the queues grow

Run it alone under ``rocprofv3 --kernel-trace --stats -- python bench/limits_trim.py ...`` and
read k_dequeue's average per launch; the script itself prints one JSON line with the host
clock's median step time and the counters it saw."""

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

QUEUES, PER_STEP, LIMIT = 16, 1000, 1024


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--limits", type=int, default=1)
    ap.add_argument("--steps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    from chanamq_amd.engine.dataplane import GpuDataPlane
    from chanamq_amd.engine.traffic import publish_command
    total = (a.steps + a.warmup) * PER_STEP
    cap = 1 << (total + LIMIT).bit_length()
    dp = GpuDataPlane(c_max=64, chpc=4, q_max=64, x_max=16, cons_max=64, seg_max=64, cmd_max=1 << 15, pair_max=1 << 15,
                      deliv_max=4096, msg_max=1 << 20, ucap=256, ingress_cap=8 << 20, egress_cap=8 << 20,
                      log_bytes=256 << 20, log_block=1 << 20, ring_pool=QUEUES * cap, tb_max=16, carry_cap=1 << 16,
                      dhash=256, req_max=256, default_queue_capacity=cap, **({"queue_limits": True} if a.limits else {}))
    vh = "AMQ.DEFAULT"
    inputs = {}
    for i in range(QUEUES):
        q = f"lq{i}"
        dp.declare_queue(vh, q, **({"max_length": LIMIT} if a.limits else {}))
        dp.open_connection(i, vh)
        dp.open_channel(i, 1)
        inputs[i] = b"".join(publish_command(1, "", q, b"%016d" % k) for k in range(PER_STEP))
    times, dropped = [], 0
    for k in range(a.warmup + a.steps):
        t0 = time.perf_counter()
        r = dp.step(inputs)
        if k >= a.warmup:
            times.append(time.perf_counter() - t0)
        dropped += r.counters.get("n_maxlen_dropped", 0)
        assert r.counters["n_ring_full"] == 0 and r.counters["n_dropped_nomem"] == 0, r.counters
    depth = [dp.message_count(q.slot) for q in dp.queues.values()]
    print(json.dumps(dict(limits=a.limits, steps=a.steps, step_ms_median=round(statistics.median(times) * 1e3, 4),
                          maxlen_dropped=int(dropped), depth_min=min(depth), depth_max=max(depth))))


if __name__ == "__main__":
    main()
