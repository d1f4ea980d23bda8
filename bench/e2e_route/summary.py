"""Medians and worst runs of an ab.sh job, and the gate of the exchange-to-exchange change:
the change's median msgs/s not below the parent's lowest run, its median p50 not above the
parent's highest.  summary.py RUNS.jsonl [OUT.json]"""
import json
import statistics
import sys

runs = [json.loads(line) for line in open(sys.argv[1]) if line.strip()]
rows = [dict(build=r["build"], msgs_per_s=r["result"]["value"], ms_per_step=r["result"]["ms_per_step"],
             p50_latency_ms=r["result"]["p50_latency_ms"], p99_latency_ms=r["result"]["p99_latency_ms"]) for r in runs]
summ = {}
for b in ("parent", "change"):
    v = [r["msgs_per_s"] for r in rows if r["build"] == b]
    p = [r["p50_latency_ms"] for r in rows if r["build"] == b]
    summ[b] = dict(runs=len(v), median_msgs_per_s=statistics.median(v), lowest_msgs_per_s=min(v),
                   median_p50_ms=statistics.median(p), highest_p50_ms=max(p))
gate = dict(throughput_ok=summ["change"]["median_msgs_per_s"] >= summ["parent"]["lowest_msgs_per_s"],
            p50_ok=summ["change"]["median_p50_ms"] <= summ["parent"]["highest_p50_ms"])
doc = dict(command="python bench.py --gpus 1 --steps 50 --warmup 10", runs=rows, summary=summ, gate=gate)
print(json.dumps(dict(summary=summ, gate=gate), indent=1))
if len(sys.argv) > 2:
    with open(sys.argv[2], "w") as f:
        json.dump(doc, f, indent=1)
