#!/usr/bin/env python3
"""What a publish caught by an alternate exchange costs: 16 connections publish 64 messages each
per step (1024 publishes) to a direct exchange ``front`` with one bound queue and the fanout
``catchall`` as its alternate exchange; a fixed share of them carries a routing key ``front``
does not know and is caught.  Both queues have an auto-ack consumer, so every step delivers what
it took.

  --share 0|10|100   per cent of the step's publishes that miss ``front``
  --mode alt         the missing share is published to ``front`` and caught by the alternate
                     (``front`` has XF_HOP: all of its publishes, hits included, are walked)
  --mode direct      the same traffic with the missing share published to ``catchall`` directly,
                     on a plane built alike (the flag on, ``front`` declared without the argument)

Without arguments the six combinations run one after the other, each in a child process of its own
under a time limit (``--limit`` seconds); the first that fails or runs out of time ends the run,
and nothing is tried twice.  Each prints one JSON line with the host clock's median step period;
the cost per caught publish is the difference of the two modes' periods at one share, divided by
the publishes caught in a step."""

import argparse
import json
import signal
import statistics
import subprocess
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

CONNS, PER_CONN, NOW = 16, 64, 1_800_000_000_000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--share", type=int, choices=(0, 10, 100), default=None)
    ap.add_argument("--mode", choices=("alt", "direct"), default="alt")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--limit", type=int, default=60, help="seconds one run may take")
    a = ap.parse_args()
    if a.share is None:
        for share in (0, 10, 100):
            for mode in ("direct", "alt"):
                cmd = [sys.executable, __file__, "--share", str(share), "--mode", mode, "--steps", str(a.steps),
                       "--warmup", str(a.warmup), "--limit", str(a.limit)]
                try:
                    rc = subprocess.run(cmd, timeout=a.limit + 15).returncode
                except subprocess.TimeoutExpired:
                    rc = 124
                if rc:
                    sys.exit(f"alternate_exchange bench: share {share} mode {mode} ended with status {rc}; "
                             "the later runs were not made")
        return
    signal.alarm(a.limit)   # a step that hangs ends this process: SIGALRM's default action
    from chanamq_amd.engine.dataplane import GpuDataPlane
    from chanamq_amd.engine.traffic import publish_command
    cap = 1 << 12
    dp = GpuDataPlane(c_max=64, chpc=4, q_max=64, x_max=16, cons_max=64, seg_max=64, cmd_max=1 << 15, pair_max=1 << 16,
                      deliv_max=4096, msg_max=1 << 20, ucap=4096, ingress_cap=16 << 20, egress_cap=8 << 20,
                      log_bytes=1 << 30, log_block=1 << 20, ring_pool=1 << 20, tb_max=16, carry_cap=1 << 16,
                      dhash=256, req_max=256, default_queue_capacity=cap, alternate_exchange=True)
    vh = "AMQ.DEFAULT"
    dp.declare_exchange(vh, "catchall", "fanout")
    dp.declare_exchange(vh, "front", "direct", arguments={"alternate-exchange": "catchall"} if a.mode == "alt" else None)
    for q, x, k in (("known", "front", "known"), ("caught", "catchall", "")):
        dp.declare_queue(vh, q)
        dp.bind(vh, q, x, k)
    dp.open_connection(40, vh)
    for ch, q in enumerate(("known", "caught"), 1):   # (a channel each: a step's deliveries fit its window)
        dp.open_channel(40, ch)
        dp.consume(40, ch, vh, q, "c-" + q, no_ack=True)
    inputs, miss = {}, 0
    for i in range(CONNS):
        dp.open_connection(i, vh)
        dp.open_channel(i, 1)
        cmds = []
        for k in range(PER_CONN):
            n = i * PER_CONN + k
            if (n * a.share) // 100 != ((n + 1) * a.share) // 100:   # evenly spread over the step
                miss += 1
                cmds.append(publish_command(1, "front", "unknown", b"%016d" % n) if a.mode == "alt"
                            else publish_command(1, "catchall", "unknown", b"%016d" % n))
            else:
                cmds.append(publish_command(1, "front", "known", b"%016d" % n))
        inputs[i] = b"".join(cmds)
    times, seen = [], dict.fromkeys(("n_alt", "n_deliv", "n_unroutable"), 0)
    for k in range(a.warmup + a.steps):
        t0 = time.perf_counter()
        r = dp.step(inputs, now_ms=NOW + 10 * k)
        if k >= a.warmup:
            times.append(time.perf_counter() - t0)
        for c in seen:
            seen[c] += int(r.counters.get(c, 0))
        assert r.counters["n_ring_full"] == 0 and r.counters["n_dropped_nomem"] == 0, r.counters
    total = a.warmup + a.steps
    backlog = sum(int(dp.message_count(q.slot)) for q in dp.queues.values())
    assert seen["n_deliv"] + backlog == total * CONNS * PER_CONN and seen["n_unroutable"] == 0, (seen, backlog)
    assert backlog <= CONNS * PER_CONN, f"the consumers fall behind: {backlog} messages queued"
    assert seen["n_alt"] == (total * miss if a.mode == "alt" else 0), seen
    print(json.dumps(dict(share=a.share, mode=a.mode, steps=a.steps, publishes_per_step=CONNS * PER_CONN,
                          caught_per_step=miss, backlog=backlog, step_ms_median=round(statistics.median(times) * 1e3, 4),
                          step_ms_min=round(min(times) * 1e3, 4), **seen)))


if __name__ == "__main__":
    main()
