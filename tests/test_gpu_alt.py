"""Alternate exchanges on the HIP data plane: the ALT instantiations of route pass 0 (k_route<true>,
k_import_route<*, true>: csrc/kernels/dataplane.hip route_one) and the x_alt table.  Every scenario
of tests/alt_scenarios.py, in the captured graph and with eager launches, judged by the scenarios'
own record and then compared step by step with the golden model: egress bytes, counters (n_alt
included) and queue depths must be equal.  Plus a 2-rank cluster on one GPU against the
single-plane oracle, and the flag off."""

import pytest
import torch  # noqa: F401  (loaded before the extension initialises HIP)

from alt_scenarios import SCENARIOS, SHARED, check, golden_plane, gpu_plane, run_alt, sp_alt_sharded, with_alts
from e2e_scenarios import assert_same
from gpu_cfg import CFG
from test_e2e_golden import assert_cluster_matches, golden, run_cluster_e2e, run_single_e2e

pytestmark = pytest.mark.gpu

MODES = {"graph": True, "eager": False}
_golden = {}


def golden_outs(sc, key, cfg):
    """The golden model's run of a scenario: computed once, only read by the cases."""
    if key not in _golden:
        g = golden_plane(cfg, **sc.flags)
        _golden[key] = run_alt(g, sc.fn(g))
    return _golden[key]


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_alt(gpu, name, mode):
    sc = SCENARIOS[name]
    cfg = dict(CFG, **sc.cfg)
    d = gpu_plane(cfg, MODES[mode], **sc.flags)
    assert d.info["alternate_exchange"] == 1
    rec = sc.fn(d)
    od = run_alt(d, rec)
    check(rec, od)
    og = golden_outs(sc, name, cfg)
    assert_same(og, od)
    for k, (a, b) in enumerate(zip(og, od)):
        for c in SHARED:
            assert a["counters"].get(c, 0) == b["counters"].get(c, 0), f"step {k}: {c}"
        assert a["depth"] == b["depth"], f"step {k}"


def test_flag_off_ignores_the_argument(gpu):
    """Built without the flag the plane reports it, keeps no n_alt and routes as it did."""
    d = gpu_plane(CFG, alternate_exchange=False)
    assert d.info["alternate_exchange"] == 0 and not d.alternate_exchange
    rec = SCENARIOS["edge_only"].fn(d)
    outs = run_alt(d, rec)
    assert all("n_alt" not in o["counters"] for o in outs)
    assert sum(o["counters"]["n_unroutable"] for o in outs) == 3 and not any(o["depth"]["qa"] for o in outs)


def test_gpu_cluster_matches_single_plane(gpu):
    from chanamq_amd.engine.dataplane import GpuDataPlane
    torch.cuda.set_device(0)
    single = run_single_e2e(sp_alt_sharded(), 2, with_alts(lambda **kw: golden(alternate_exchange=True, **kw),
                                                           sp_alt_sharded()))
    make = lambda **kw: GpuDataPlane(alternate_exchange=True, **CFG, **kw)
    _, clus = run_cluster_e2e(sp_alt_sharded(), 2, with_alts(make, sp_alt_sharded()))
    assert_cluster_matches(single, clus)


def test_host_assembled_publish_is_caught(gpu):
    """publish_host (a message larger than the carry, world 1): routed on the device by the import
    path's pass 0, whose ALT instantiation follows the alternate as well."""
    from alt_scenarios import Rec
    from chanamq_amd.protocol.codec import encode_properties
    from dp_scenarios import VH
    d = gpu_plane(CFG)
    r = Rec(d)
    r.x("ca", "fanout")
    r.x("front", "direct", alt="ca")
    r.x("hole", "direct", alt="absent")
    r.q("qca", [("ca", "")], consume=False)
    r.q("qk", [("front", "k")], consume=False)
    depth = lambda q: d.message_count(d.queues[(VH, q)].slot)
    props, body = encode_properties({"delivery_mode": 1}), b"b" * 300
    assert d.publish_host(1, 1, r.slot("front"), b"front", b"missing", props, body, 0, now_ms=10) == 1
    assert (depth("qca"), depth("qk")) == (1, 0)
    assert d.publish_host(1, 1, r.slot("front"), b"front", b"k", props, body, 0, now_ms=11) == 1
    assert (depth("qca"), depth("qk")) == (1, 1)
    assert d.publish_host(1, 1, r.slot("hole"), b"hole", b"k", props, body, 0, now_ms=12) == 0
