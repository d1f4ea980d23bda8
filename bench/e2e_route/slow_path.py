"""Step time of the `wide` scenario shape scaled to a few thousand publishes: 40 distinct
queues reached through two exchange-to-exchange branches that share 10, against the same
publishes to a fanout exchange bound to the 40 queues directly.  One JSON line."""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from chanamq_amd.engine.dataplane import GpuDataPlane  # noqa: E402
from chanamq_amd.engine.traffic import publish_stream  # noqa: E402

VH = "AMQ.DEFAULT"
N, CONNS = 2048, 8
dp = GpuDataPlane(c_max=64, chpc=8, q_max=64, x_max=64, cons_max=256, seg_max=64, cmd_max=32768, deliv_max=4096,
                  msg_max=1 << 18, ucap=256, ingress_cap=8 << 20, egress_cap=16 << 20, log_bytes=256 << 20,
                  log_block=1 << 20, ring_pool=1 << 23, default_queue_capacity=1 << 17, tb_max=64,
                  carry_cap=1 << 20, dhash=1024, req_max=4096)
for x, t in (("wa", "fanout"), ("wb", "fanout"), ("wc", "direct"), ("flat", "fanout")):
    dp.declare_exchange(VH, x, t)
dp.bind_exchange(VH, "wb", "wa", "")
dp.bind_exchange(VH, "wc", "wa", "")
for i in range(40):
    q = f"w{i:02d}"
    dp.declare_queue(VH, q)
    if i < 25:
        dp.bind(VH, q, "wb", "")
    if i >= 15:
        dp.bind(VH, q, "wc", "k")
    dp.bind(VH, q, "flat", "")
for c in range(CONNS):
    dp.open_connection(c, VH)
    dp.open_channel(c, 1)
inputs = {ex: {c: publish_stream(N // CONNS, ex, lambda i: "k", 48, seed=c) for c in range(CONNS)}
          for ex in ("wa", "flat")}
times = {"wa": [], "flat": []}
for rnd in range(8):
    for ex in ("wa", "flat"):
        r = dp.step(inputs[ex])
        assert r.counters["n_pairs"] == N * 40, (ex, r.counters["n_pairs"])
        if rnd >= 2:
            times[ex].append(r.elapsed * 1e3)
out = dict(publishes_per_step=N, queues_per_publish=40, body_bytes=48,
           hop_step_ms=times["wa"], direct_step_ms=times["flat"],
           hop_median_ms=statistics.median(times["wa"]), direct_median_ms=statistics.median(times["flat"]))
print(json.dumps(out))
if len(sys.argv) > 1:   # also written to the file named on the command line
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=1)
