#!/usr/bin/env python3
"""H, C, delta and the copy engine's idle gap of a bench.py run, from a rocprofv3 kernel +
memory-copy trace written as csv (profiles/link_rate/model.md).

usage: trace_model.py TRACE_DIR [timed_steps]

  H      a step's payload copy: first half's start to last half's end
  C      max(copy end, start of the first kernel behind the ingress wait) to the end of k_post
  delta  end of k_post of step i-1 to the start of step i+1's payload copy
  idle   end of step i's payload copy to the start of step i+1's
  P      payload copy start to payload copy start
Medians over the last `timed_steps` steps (default 50), the final two left out (pipeline drain).
"""
import csv
import glob
import json
import statistics
import sys


def rows(d, pat):
    f = glob.glob(f"{d}/**/*{pat}*.csv", recursive=True)
    if not f:
        raise SystemExit(f"no *{pat}*.csv under {d}")
    with open(f[0], newline="") as fh:
        return list(csv.DictReader(fh))


def main(d, timed=50):
    ks = sorted(((r["Kernel_Name"].split("(")[0].replace("void ", ""), int(r["Start_Timestamp"]), int(r["End_Timestamp"]))
                 for r in rows(d, "kernel_trace")), key=lambda k: k[1])
    cp = sorted(((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r.get("Direction", "")) for r in rows(d, "memory_copy_trace")),
                key=lambda c: c[0])
    # payload copies: host-to-device and long (the descriptors and Get requests are microseconds)
    pay = [c for c in cp if "HOST_TO_DEVICE" in c[2].upper().replace("2", "_TO_") and c[1] - c[0] > 50_000]
    groups = []   # halves of one payload start within 30 us of each other
    for c in pay:
        if groups and c[0] - groups[-1][0][0] < 30_000:
            groups[-1].append(c)
        else:
            groups.append([c])
    copies = [(min(c[0] for c in g), max(c[1] for c in g), len(g)) for g in groups]
    steps = []    # one per k_stage: {kernel name: (start, end)}
    for n, s, e in ks:
        if n.startswith("k_stage"):
            steps.append({})
        if steps:
            steps[-1].setdefault(n, (s, e))
            steps[-1]["_sum"] = steps[-1].get("_sum", 0) + (e - s)
            steps[-1]["_n"] = steps[-1].get("_n", 0) + 1
    steps = [s for s in steps if any(n.startswith("k_post") for n in s)]
    # a step's payload: the last one complete before its frame scan ends (the scan, or the
    # wait in front of it, holds the step until the copy is done); steps without one are left out
    head_of = lambda s: next(v for k, v in s.items() if k.startswith("k_frame_scan"))
    paired = []
    for s in steps:
        mine = [c for c in copies if c[1] <= head_of(s)[1]]
        if mine and (not paired or mine[-1] is not paired[-1][1]):
            paired.append((s, mine[-1]))
    steps, copies = [p[0] for p in paired], [p[1] for p in paired]
    n = len(steps)
    post = [next(v for k, v in s.items() if k.startswith("k_post")) for s in steps]
    head = [head_of(s) for s in steps]
    lo, hi = max(2, n - timed), n - 2
    us = lambda x: round(statistics.median(x) / 1e3, 1)
    out = {
        "steps": hi - lo,
        "halves_per_payload": statistics.median(c[2] for c in copies[lo:hi]),
        "H_us": us([copies[i][1] - copies[i][0] for i in range(lo, hi)]),
        "C_us": us([post[i][1] - max(copies[i][1], head[i][0]) for i in range(lo, hi)]),
        "delta_us": us([copies[i + 1][0] - post[i - 1][1] for i in range(lo, hi - 1)]),
        "copy_idle_us": us([copies[i + 1][0] - copies[i][1] for i in range(lo, hi - 1)]),
        "P_us": us([copies[i + 1][0] - copies[i][0] for i in range(lo, hi - 1)]),
        "kernel_sum_us": us([steps[i]["_sum"] for i in range(lo, hi)]),
        "kernels_per_step": statistics.median(steps[i]["_n"] for i in range(lo, hi)),
        "copy_end_to_post_end_us": us([post[i][1] - copies[i][1] for i in range(lo, hi)]),
        "per_kernel_us": {k: us([steps[i][k][1] - steps[i][k][0] for i in range(lo, hi) if k in steps[i]])
                          for k in steps[hi - 1] if not k.startswith("_")},
    }
    H, C, dl = out["H_us"], out["C_us"], out["delta_us"]
    out["model_P_us"] = round(max(H, (H + C + dl) / 2), 1)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main(sys.argv[1], int(sys.argv[2]) if len(sys.argv) > 2 else 50)
