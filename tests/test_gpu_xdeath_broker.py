"""x-death headers and cycle detection through the server on the HIP data plane: the conversation of
tests/xdeath_broker_script.py against ``GpuBroker(dead_letter=True, x_death=True)`` over a
``GpuDataPlane`` built alike, with the Python-stepped and the pipelined front end (whose statistics
carry dl_cycle from the step's counters)."""

import pytest

from gpu_cfg import CFG
from test_xdeath_broker import serve
from xdeath_broker_script import xdeath_script

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("io", ["native", "pipeline"])
def test_x_death_on_gpu_plane(gpu, io):
    from chanamq_amd.engine.dataplane import GpuDataPlane
    plane = GpuDataPlane(**dict(CFG, default_queue_capacity=1 << 12, dead_letter=True, x_death=True))
    b = serve(plane, io, dead_letter=True, x_death=True)
    try:
        xdeath_script(b)
    finally:
        b.stop()
