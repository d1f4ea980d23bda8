"""Dead-lettering through the server on the HIP data plane: the conversations of
tests/dlx_broker_script.py against ``GpuBroker(dead_letter=True)`` over a
``GpuDataPlane(dead_letter=True)``, with the Python-stepped and the pipelined front end."""

import pytest

from dlx_broker_script import dlx_script, off_script, refusals_script
from gpu_cfg import CFG
from test_dlx_broker import serve

pytestmark = pytest.mark.gpu


def plane(on=True, **kw):
    from chanamq_amd.engine.dataplane import GpuDataPlane
    cfg = dict(CFG, default_queue_capacity=1 << 12, **kw)
    if on:
        cfg.update(dead_letter=True)
    return GpuDataPlane(**cfg)


@pytest.mark.parametrize("io", ["native", "pipeline"])
def test_dead_letter_on_gpu_plane(gpu, io):
    b = serve(plane(), io, dead_letter=True)
    try:
        dlx_script(b)
    finally:
        b.stop()


def test_invalid_arguments_are_406(gpu):
    b = serve(plane(), "native", dead_letter=True)
    try:
        refusals_script(b)
    finally:
        b.stop()


def test_option_off_ignores_the_arguments(gpu):
    b = serve(plane(on=False), "native")
    try:
        off_script(b)
    finally:
        b.stop()
