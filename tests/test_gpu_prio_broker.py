"""Priority queues through the server on the HIP data plane: the conversations of
tests/prio_broker_script.py against ``GpuBroker(priority_queues=True)`` over a ``GpuDataPlane``
built with it, with the Python-stepped and the pipelined front end."""

import pytest

from gpu_cfg import CFG
from prio_broker_script import off_script, priority_script, refusals_script
from test_prio_broker import ON, serve

pytestmark = pytest.mark.gpu


def plane(on=True, **kw):
    from chanamq_amd.engine.dataplane import GpuDataPlane
    return GpuDataPlane(**dict(CFG, default_queue_capacity=1 << 12, **kw), **(ON if on else {}))


@pytest.mark.parametrize("io", ["native", "pipeline"])
def test_priorities_on_gpu_plane(gpu, io):
    b = serve(plane(), io, **ON)
    try:
        priority_script(b)
    finally:
        b.stop()


def test_refusals_are_406(gpu):
    b = serve(plane(), "native", **ON)
    try:
        refusals_script(b)
    finally:
        b.stop()


def test_flag_off_ignores_the_argument(gpu):
    p = plane(on=False)
    assert p.info["priority_queues"] == 0
    b = serve(p, "native")
    try:
        off_script(b)
    finally:
        b.stop()


def test_flag_is_single_rank_only(gpu):
    from chanamq_amd.engine.dataplane import GpuDataPlane
    with pytest.raises(ValueError):
        GpuDataPlane(**dict(CFG, priority_queues=True, world=2))
