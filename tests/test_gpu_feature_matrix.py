"""Every combination of the opt-in features that selects a different set of kernel launches
(csrc/kernels/engine.hip: ``with_flags`` in launch_route, launch_tail, launch_dead and basic_get),
each against the golden model built with the same flags.

The scenarios declare no feature argument, so every plane has to answer as the all-off plane does
(tests/test_features.py holds the golden model to that); between them they run route and
route_store, the enqueue path, chan_advance, dequeue with requeue, the dead pass where it is on,
and Basic.Get between steps."""

import functools
import itertools

import pytest

from dp_scenarios import SCENARIOS, run
from gpu_cfg import CFG

pytestmark = pytest.mark.gpu

NAMES = ("headers_match", "queue_limits", "queue_limit_bytes", "priority_queues", "dead_letter", "x_death",
         "alternate_exchange")
MATRIX_SCENARIOS = ("nack_requeue", "basic_get", "ttl", "confirm_mandatory")


def flags(bits):
    return dict(zip(NAMES, (c == "1" for c in bits)))


# (queue_limits, queue_limit_bytes) x priority_queues x (dead_letter, x_death) x alternate_exchange,
# headers_match off; and all on / all off with headers_match on
COMBOS = ["0" + ql + p + dl + a for ql, p, dl, a in itertools.product(("00", "10", "11"), "01", ("00", "10", "11"), "01")]
COMBOS += ["1000000", "1111111"]
assert len(COMBOS) == 38 and len(set(COMBOS)) == 38


@functools.lru_cache(maxsize=None)
def golden_outputs(bits, name):
    from chanamq_amd.engine.golden import GoldenDataPlane
    g = GoldenDataPlane(c_max=CFG["c_max"], chpc=CFG["chpc"], q_max=CFG["q_max"], x_max=CFG["x_max"],
                        cons_max=CFG["cons_max"], ucap=CFG["ucap"], carry_cap=CFG["carry_cap"],
                        default_queue_capacity=CFG["default_queue_capacity"], **flags(bits))
    return run(g, SCENARIOS[name](g), now_step_ms=3000)


def check(bits, name, graph):
    from chanamq_amd.engine.dataplane import GpuDataPlane
    f = flags(bits)
    d = GpuDataPlane(graph=graph, **CFG, **f)
    for n in NAMES[1:]:
        assert d.info[n] == int(f[n]), n
    assert {n: getattr(d, n) for n in NAMES} == f
    od = run(d, SCENARIOS[name](d), now_step_ms=3000)
    og = golden_outputs(bits, name)
    assert len(og) == len(od)
    for k, (a, b) in enumerate(zip(og, od)):
        assert a["segs"] == b["segs"], f"step {k} segs"
        assert a["ctrl"] == b["ctrl"], f"step {k} ctrl"
        assert a["events"] == b["events"], f"step {k} events"
        assert a["gets"] == b["gets"], f"step {k} basic.get"
        assert a["txbuf"] == b["txbuf"], f"step {k} tx-held commands"
        assert sorted(a["egress"]) == sorted(b["egress"]), f"step {k} egress conns"
        for c in a["egress"]:
            assert a["egress"][c] == b["egress"][c], f"step {k} conn {c} egress differs"


@pytest.mark.parametrize("name", MATRIX_SCENARIOS)
@pytest.mark.parametrize("bits", COMBOS)
def test_feature_combination_matches_golden(gpu, bits, name):
    check(bits, name, graph=True)


@pytest.mark.parametrize("name", MATRIX_SCENARIOS)
@pytest.mark.parametrize("bits", ["0000000", "1111111"])
def test_eager_launches_match_golden(gpu, bits, name):
    check(bits, name, graph=False)
