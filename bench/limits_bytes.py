#!/usr/bin/env python3
"""What the byte limit costs a step: 16 queues without consumers, each taking 1000 publishes a
step (16 connections x 1000, 16-byte bodies, default exchange), in three workloads.

  --mode trim     drop-head queues with x-max-length-bytes = 16 KiB: from the second step on every
                  queue trims about 1000 entries by bytes at the end of each step
  --mode reject   reject-publish queues with the same limit: from the second step on k_byte_room
                  finds K = 0 or little more and every queue refuses about 1000 pairs a step
  --mode reject-count   for comparison: reject-publish queues with x-max-length = 1024 and no byte
                  limit, which refuse the same pairs through the refusal path both limits share
  --mode none     the same traffic and no limited queue: what the ready-bytes bookkeeping and the
                  materialised sort path cost alone (the queues grow)

  --bytes 1       the plane is built with queue_limit_bytes (the queues carry the limit)
  --bytes 0       the same plane and traffic with the flag off: the argument is ignored, the step
                  sorts its pairs on the fused one-pass path, the queues grow

Run it alone under ``rocprofv3 --kernel-trace --stats -- python bench/limits_bytes.py ...`` and
read the per-launch averages of k_byte_room, k_dequeue and the enqueue kernels; the script itself
prints one JSON line with the host clock's median step time and the counters it saw."""

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

QUEUES, PER_STEP, BODY, LIMIT_BYTES = 16, 1000, 16, 16 << 10
MODES = {"trim": "drop-head", "reject": "reject-publish", "reject-count": "reject-publish", "none": None}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=sorted(MODES), default="trim")
    ap.add_argument("--bytes", type=int, default=1)
    ap.add_argument("--steps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    from chanamq_amd.engine.dataplane import GpuDataPlane
    from chanamq_amd.engine.traffic import publish_command
    total = (a.steps + a.warmup) * PER_STEP
    cap = 1 << (total + LIMIT_BYTES // BODY).bit_length()
    dp = GpuDataPlane(c_max=64, chpc=4, q_max=64, x_max=16, cons_max=64, seg_max=64, cmd_max=1 << 15, pair_max=1 << 15,
                      deliv_max=4096, msg_max=1 << 20, ucap=256, ingress_cap=8 << 20, egress_cap=8 << 20,
                      log_bytes=256 << 20, log_block=1 << 20, ring_pool=QUEUES * cap, tb_max=16, carry_cap=1 << 16,
                      dhash=256, req_max=256, default_queue_capacity=cap, queue_limits=True,
                      **({"queue_limit_bytes": True} if a.bytes else {}))
    vh = "AMQ.DEFAULT"
    inputs = {}
    mode = MODES[a.mode]
    for i in range(QUEUES):
        q = f"bq{i}"
        lim = {"max_length": LIMIT_BYTES // BODY} if a.mode == "reject-count" else {"max_length_bytes": LIMIT_BYTES}
        dp.declare_queue(vh, q, **(dict(lim, overflow=mode) if mode else {}))
        dp.open_connection(i, vh)
        dp.open_channel(i, 1)
        inputs[i] = b"".join(publish_command(1, "", q, b"%016d" % k) for k in range(PER_STEP))
    times, dropped, rejected = [], 0, 0
    for k in range(a.warmup + a.steps):
        t0 = time.perf_counter()
        r = dp.step(inputs)
        if k >= a.warmup:
            times.append(time.perf_counter() - t0)
        dropped += r.counters.get("n_maxlen_dropped", 0)
        rejected += r.counters.get("n_maxlen_rejected", 0)
        assert r.counters["n_ring_full"] == 0 and r.counters["n_dropped_nomem"] == 0, r.counters
    depth = [dp.message_count(q.slot) for q in dp.queues.values()]
    out = dict(mode=a.mode, bytes=a.bytes, steps=a.steps, step_ms_median=round(statistics.median(times) * 1e3, 4),
               maxlen_dropped=int(dropped), maxlen_rejected=int(rejected), depth_min=min(depth), depth_max=max(depth))
    if a.bytes:
        nb = [dp.queue_bytes(q.slot) for q in dp.queues.values()]
        out.update(ready_bytes_min=int(min(nb)), ready_bytes_max=int(max(nb)))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
