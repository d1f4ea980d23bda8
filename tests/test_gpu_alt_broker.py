"""Alternate exchanges through the server on the HIP data plane: the conversation of
tests/alt_broker_script.py against ``GpuBroker(alternate_exchange=True)`` over a ``GpuDataPlane``
built alike, with the Python-stepped and the pipelined front end (whose statistics carry alt_routed
from the step's counters)."""

import pytest

from alt_broker_script import alt_script
from gpu_cfg import CFG
from test_xdeath_broker import serve

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("io", ["native", "pipeline"])
def test_alternate_exchange_on_gpu_plane(gpu, io):
    from chanamq_amd.engine.dataplane import GpuDataPlane
    plane = GpuDataPlane(**dict(CFG, default_queue_capacity=1 << 12, alternate_exchange=True))
    b = serve(plane, io, alternate_exchange=True)
    try:
        alt_script(b)
    finally:
        b.stop()
