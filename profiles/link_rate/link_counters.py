#!/usr/bin/env python3
"""The ingress engines and the split / unsplit payload-copy counts of the bench's default
shape (config 2: 256 producers x 49152 B per step), which bench.py's result line cannot
show.  Run from the repository root: python profiles/link_rate/link_counters.py [steps]"""
import json
import os
import sys

sys.path.insert(0, os.getcwd())

import bench  # noqa: E402
from chanamq_amd.engine.dataplane import GpuDataPlane  # noqa: E402


def main(steps=12):
    P, Q, chunk, blocks = 256, 16, 49152, 8
    cfg = dict(c_max=max(1024, P + Q + 1), chpc=4, q_max=Q + 64, cons_max=1024, seg_max=1024, cmd_max=1 << 17,
               deliv_max=1 << 16, msg_max=1 << 22, ucap=4096, deliver_cap=8192, ingress_cap=32 << 20,
               egress_cap=128 << 20, log_bytes=16 << 30, ring_pool=Q * (1 << 20) + Q + 1024, tb_max=64,
               fan_max=1 << 20, carry_cap=256 << 10, graph=1, copy_engine=3, sdma_engine=-1, sdma_split=1,
               egress_gate=1, overlap=0, parities=2, h2d_alt=0, h2d_hsa=1, egress_ref=0)   # as bench.py's defaults
    dp = GpuDataPlane(device=0, worker=0, **cfg)
    pool, segs, offs, blens, *_ = bench.build_workload(dp, 0, P, Q, 1024, chunk, blocks, cons_base=P)
    base = pool.ctypes.data
    pending = []
    for i in range(steps):
        b = i % blocks
        pending.append(dp.submit_raw(segs[b], base + offs[b], blens[b]))
        if len(pending) > 1:
            t = pending.pop(0)
            dp.wait(t)
            if i + 1 < steps:   # the next payload right behind the wait, as the bench queues it
                nb = (i + 1) % blocks
                dp.prefetch(base + offs[nb], blens[nb])
            dp.finish(t, collect=False, waited=True)
    for t in pending:
        dp.finish(t, collect=False)
    info = dp.info
    print(json.dumps({
        "steps": steps, "payload_bytes": sorted(set(int(x) for x in blens)),
        "h2d_split_min": info["h2d_split_min"],
        "engines": {k: info[k] for k in ("sdma_engine", "egress_tail_engine", "h2d_hsa_engine", "h2d_hsa_engine2")},
        "h2d_stats": dp.h2d_stats()}, indent=1))


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 12)
