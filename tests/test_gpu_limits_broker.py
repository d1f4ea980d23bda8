"""Queue length limits through the server on the HIP data plane: the conversations of
tests/limits_broker_script.py against ``GpuBroker(queue_limits=True)`` over a
``GpuDataPlane(queue_limits=True)``, with the Python-stepped and the pipelined front end."""

import pytest

from gpu_cfg import CFG
from limits_broker_script import durable_after, durable_before, limits_script, off_script, refusals_script
from test_limits_broker import serve

pytestmark = pytest.mark.gpu


def plane(on=True, **kw):
    from chanamq_amd.engine.dataplane import GpuDataPlane
    cfg = dict(CFG, default_queue_capacity=1 << 12, **kw)
    if on:
        cfg.update(queue_limits=True)
    return GpuDataPlane(**cfg)


@pytest.mark.parametrize("io", ["native", "pipeline"])
def test_limits_on_gpu_plane(gpu, io):
    b = serve(plane(), io, queue_limits=True)
    try:
        limits_script(b)
    finally:
        b.stop()


def test_invalid_arguments_are_406(gpu):
    b = serve(plane(), "native", queue_limits=True)
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


def test_recovered_durable_queue_adopts_a_limit(gpu, tmp_path):
    from chanamq_amd.broker import load
    core = load()

    def boot():
        st = core.Store()
        st.open(str(tmp_path / "store"), True)
        p = plane(persist=1, persist_max=4096, persist_bytes=8 << 20, restore_max=1024, restore_bytes=8 << 20)
        return st, serve(p, "native", store=st, queue_limits=True)
    st, b = boot()
    try:
        durable_before(b.port)
    finally:
        b.stop()
        st.close()
    st, b = boot()
    try:
        durable_after(b)
    finally:
        b.stop()
        st.close()
