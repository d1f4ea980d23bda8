"""Queue byte limits through the server on the HIP data plane: the conversations of
tests/bytelimits_broker_script.py against ``GpuBroker(queue_limits=True, queue_limit_bytes=True)``
over a ``GpuDataPlane`` built with both, with the Python-stepped and the pipelined front end."""

import pytest

from bytelimits_broker_script import bytelimits_script, off_script, refusals_script
from gpu_cfg import CFG
from test_bytelimits_broker import ON, serve

pytestmark = pytest.mark.gpu


def plane(on=True, **kw):
    from chanamq_amd.engine.dataplane import GpuDataPlane
    return GpuDataPlane(**dict(CFG, default_queue_capacity=1 << 12, **kw), **(ON if on else {"queue_limits": True}))


@pytest.mark.parametrize("io", ["native", "pipeline"])
def test_bytelimits_on_gpu_plane(gpu, io):
    b = serve(plane(), io, **ON)
    try:
        bytelimits_script(b)
    finally:
        b.stop()


def test_invalid_arguments_are_406(gpu):
    b = serve(plane(), "native", **ON)
    try:
        refusals_script(b)
    finally:
        b.stop()


def test_flag_off_ignores_the_argument(gpu):
    p = plane(on=False)
    assert p.info["queue_limits"] == 1 and p.info["queue_limit_bytes"] == 0
    b = serve(p, "native", queue_limits=True)
    try:
        off_script(b)
    finally:
        b.stop()


def test_flag_needs_queue_limits(gpu):
    from chanamq_amd.engine.dataplane import GpuDataPlane
    with pytest.raises(ValueError):
        GpuDataPlane(**dict(CFG, queue_limit_bytes=True))
