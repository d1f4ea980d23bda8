#!/usr/bin/env python3
"""What dead-lettering costs a step with the flag on: 16 queues with a dead-letter exchange and
no consumers, one parking queue behind a fanout exchange, 16 connections publishing to them.

  --mode idle    the flag on and nothing dying: the dead pass's six launches find an empty list
  --mode dying   every step `dead_max` (1024) entries expire at the heads (64 per queue, published
                 the step before with a 1 ms expiration and a clock that advances 10 ms a step),
                 and the step's dead pass publishes the 1024 of the step before
  --mode off     the same traffic on a plane built without the flag (the arguments are ignored)

Without ``--mode`` the three modes run one after the other, each in a child process of its own
under a time limit (``--limit`` seconds); the first that fails or runs out of time ends the run,
and nothing is tried twice.  With ``--mode`` one mode runs in this process, under the same limit
(an alarm ends it): that is the form to put under
``rocprofv3 --kernel-trace --stats -f csv -- python bench/dead_letter.py --mode dying`` to read
k_dead_pack, k_import_route, k_scan_route and k_route_store per launch.  Each mode prints one JSON
line with the host clock's median step period and the counters it saw."""

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
    ap.add_argument("--mode", choices=("idle", "dying", "off"), default=None)
    ap.add_argument("--steps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--limit", type=int, default=90, help="seconds one mode may take")
    a = ap.parse_args()
    if a.mode is None:   # every mode in a child of its own, under its own time limit; stop at the first failure
        for mode in ("off", "idle", "dying"):
            cmd = [sys.executable, __file__, "--mode", mode, "--steps", str(a.steps), "--warmup", str(a.warmup),
                   "--limit", str(a.limit)]
            try:
                rc = subprocess.run(cmd, timeout=a.limit + 15).returncode
            except subprocess.TimeoutExpired:
                rc = 124
            if rc:
                sys.exit(f"dead_letter bench: mode {mode} ended with status {rc}; the later modes were not run")
        return
    signal.alarm(a.limit)   # a step that hangs ends this process: SIGALRM's default action
    from chanamq_amd.engine.dataplane import GpuDataPlane
    from chanamq_amd.engine.traffic import publish_command
    on = a.mode != "off"
    cap = 1 << 17
    dp = GpuDataPlane(c_max=64, chpc=4, q_max=64, x_max=16, cons_max=64, seg_max=64, cmd_max=1 << 15, pair_max=1 << 16,
                      deliv_max=4096, msg_max=1 << 20, ucap=256, ingress_cap=8 << 20, egress_cap=8 << 20,
                      log_bytes=256 << 20, log_block=1 << 20, ring_pool=(QUEUES + 1) * cap, tb_max=16, carry_cap=1 << 16,
                      dhash=256, req_max=256, default_queue_capacity=cap, restore_max=1024,
                      **({"dead_letter": True, "dead_max": 1024, "dead_bytes": 1 << 20} if on else {}))
    vh = "AMQ.DEFAULT"
    dp.declare_exchange(vh, "dlx", "fanout")
    dp.declare_queue(vh, "park")
    dp.bind(vh, "park", "dlx", "")
    props = {"expiration": "1"} if a.mode != "idle" else None
    inputs = {}
    for i in range(QUEUES):
        q = f"dq{i}"
        dp.declare_queue(vh, q, dead_letter_exchange="dlx")
        dp.open_connection(i, vh)
        dp.open_channel(i, 1)
        inputs[i] = b"".join(publish_command(1, "", q, b"%016d" % k, props) for k in range(PER_Q))
    times, seen = [], dict.fromkeys(("n_expired", "n_dl_expired", "n_dl_unrouted", "n_dl_dropped"), 0)
    for k in range(a.warmup + a.steps):
        t0 = time.perf_counter()
        r = dp.step(inputs, now_ms=NOW + 10 * k)
        if k >= a.warmup:
            times.append(time.perf_counter() - t0)
        for c in seen:
            seen[c] += int(r.counters.get(c, 0))
        assert r.counters["n_ring_full"] == 0 and r.counters["n_dropped_nomem"] == 0, r.counters
    print(json.dumps(dict(mode=a.mode, steps=a.steps, step_ms_median=round(statistics.median(times) * 1e3, 4),
                          parked=int(dp.message_count(dp.queues[(vh, "park")].slot)),
                          pending=int(r.counters.get("n_dl_pending", 0)), **seen)))


if __name__ == "__main__":
    main()
