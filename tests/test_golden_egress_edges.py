"""The delivery-layout, connection-layout, render and persist-pack scenarios of
tests/egress_scenarios.py on the golden model (CPU), judged by ``egress_scenarios.check_run``:
the bytes every connection must receive, rendered by the scenario's own record with the host
codec.  This holds the model to the checks, proves every placement assertion of the scenarios
(they run while a scenario is built) and shows that the inputs are sound.
tests/test_gpu_egress_edges.py holds the HIP data plane to the same checks, with the counters
only it keeps, and to byte equality with this model."""

import copy

import pytest

from chanamq_amd.protocol.codec import Method, render_command
from egress_scenarios import (CONN_PASS, DELIV_PASS, DELIV_PUBLISHERS, HEADERS, PERSIST, RUN_CONS, RUN_QUEUES, SCENARIOS,
                              WIDE, WIDE_BASE, check_bytes, check_persist, check_run, check_wire, command, env_of,
                              golden_plane, limits, run_egress, same_copies, wide_cfg)
from gpu_cfg import CFG

# (the model's run of deliv_passes does not depend on egress by reference: once)
ON_MODEL = sorted(n for n in SCENARIOS if n != "deliv_passes_inline")


def run_golden(sc, cfg=None):
    cfg = dict(CFG, **(sc.cfg if cfg is None else cfg))
    g = golden_plane(cfg)
    run = sc.fn(g, limits(), env_of(g, cfg))
    return g, run, run_egress(g, run.steps, persist=bool(cfg.get("persist")))


@pytest.mark.parametrize("name", ON_MODEL)
def test_golden_passes_the_checks(name):
    g, run, outs = run_golden(SCENARIOS[name])
    assert run.placed                        # every scenario records what it asserted
    check_run(run, outs, golden=True)


def test_golden_passes_the_wide_layout():
    """c_max CONN_LAYOUT_MAX + 2, and the same traffic at c_max 64: copy k of the four-region
    connection gets the same bytes at both."""
    _, wide, ow = run_golden(WIDE, wide_cfg(limits()))
    _, base, ob = run_golden(WIDE_BASE)
    check_run(wide, ow, golden=True)
    check_run(base, ob, golden=True)
    same_copies(wide, ow, base, ob)


def test_golden_passes_the_persist_checks():
    g, run, outs = run_golden(PERSIST)
    check_run(run, outs, golden=True)
    check_persist(run, outs)
    assert sum(len(o["persist"]) for o in outs) == run.placed["records"]


def test_limits_come_from_the_build():
    """A scenario aims at these: a constant that moves takes the scenario with it, and one
    that leaves the build fails here."""
    lim = limits()
    assert RUN_CONS < lim.DVW_LDS < RUN_QUEUES * RUN_CONS            # runs_lds can grant DVW_LDS + 1 runs
    assert CONN_PASS < lim.CONN_LAYOUT_MAX and lim.CONN_LAYOUT_MAX % CONN_PASS == 0
    assert lim.RC_RET_BLOCKS * 4 + 1 <= CFG["cmd_max"]                # return_flood's publishes fit one step
    assert 2 <= lim.RD_G <= 64 and 64 % lim.RD_G == 0 and lim.RD_G + 1 < 255
    assert DELIV_PASS + 16 <= SCENARIOS["deliv_passes"].cfg["deliv_max"]
    from chanamq_amd import ops                     # a publisher's three frames per message, below the scan's limit
    assert 3 * ((DELIV_PASS + 16) // DELIV_PUBLISHERS + 1) < ops.load().FS_CAND_STAGED


def test_command_is_render_command():
    """The record's renderer is the codec's: ``command`` only keeps header frames."""
    big = dict(HEADERS, message_id="x" * 30)
    for fm in (4096, 131072):
        for size in (0, 1, fm - 9, fm - 8, fm - 7, 2 * (fm - 8) + 1):
            for props in ({}, big):
                body = bytes(range(256)) * (size // 256) + bytes(size % 256)
                for m in (Method("basic.deliver", consumer_tag="t", delivery_tag=7, redelivered=True, exchange="e",
                                 routing_key="k"),
                          Method("basic.return", reply_code=312, reply_text="r", exchange="", routing_key="k"),
                          Method("basic.get_ok", delivery_tag=1, redelivered=False, exchange="", routing_key="q",
                                 message_count=3)):
                    for _ in range(2):      # (the second time from the kept header)
                        assert command(5, m, props, body, fm) == render_command(5, m, props, body, fm)
    m = Method("basic.ack", delivery_tag=9, multiple=True)
    assert command(3, m) == render_command(3, m)


def damaged(outs, step, conn, fn):
    out = copy.deepcopy(outs)
    out[step]["egress"][conn] = fn(bytes(out[step]["egress"][conn]))
    return out


def test_the_checks_see_a_wrong_byte():
    """What the checks are for: a shifted body byte, two confirm frames in channel-number
    order, a delivery tag that starts over, a lost GetEmpty -- each fails them."""
    g, run, outs = run_golden(SCENARIOS["conn_regions_last"])
    check_run(run, outs, golden=True)
    data = bytes(outs[1]["egress"][7])
    cuts = [i for i in range(len(data) - 21) if data[i] == 1 and data[i + 3:i + 11] == b"\x00\x00\x00\x0d\x00\x3c\x00\x50"]
    assert len(cuts) == 2 and cuts[1] == cuts[0] + 21          # the two Basic.Ack frames, back to back
    a = cuts[0]
    swapped = lambda d: d[:a] + d[a + 21:a + 42] + d[a:a + 21] + d[a + 42:]
    for fn in (lambda d: d[:-40] + bytes([d[-40] ^ 1]) + d[-39:], swapped, lambda d: d[:-13], lambda d: d + d[-13:]):
        with pytest.raises(AssertionError):
            check_bytes(run, damaged(outs, 1, 7, fn))
    with pytest.raises(AssertionError):                         # the second Ack's tag (3 publishes) one short
        check_wire(run, damaged(outs, 1, 7, lambda d: d[:a + 39] + b"\x02" + d[a + 40:]))
    first = outs[1]["egress"][7].index(b"\x00\x3c\x00\x3c")    # the first Basic.Deliver: its tag, 0 for 1
    at = first + 4 + 1 + len("inline-0") + 7
    assert data[at] == 1
    with pytest.raises(AssertionError):
        check_wire(run, damaged(outs, 1, 7, lambda d: d[:at] + b"\x00" + d[at + 1:]))
