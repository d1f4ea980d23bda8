"""x-death headers and cycle detection on the golden model (CPU): every scenario of
tests/xdeath_scenarios.py, judged by the scenarios' own record (``xdeath_scenarios.check``: the
expected property bytes built from dicts through protocol/codec.py, never the model's rewrite).
tests/test_gpu_xdeath.py holds the HIP data plane to the same record and to byte equality with this
model.  Plus the construction rule."""

import pytest

from gpu_cfg import CFG
from xdeath_scenarios import SCENARIOS, check, golden_plane, run_xd


@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_golden_keeps_the_rules(name):
    sc = SCENARIOS[name]
    g = golden_plane(dict(CFG, **sc.cfg))
    rec = sc.fn(g)
    check(rec, run_xd(g, rec))
    if sc.drained:
        assert g.memory_in_use() == 0 and all(g.message_count(q.slot) == 0 for q in g.queues.values())
        assert not g.dead


def test_x_death_needs_dead_letter():
    from chanamq_amd.engine.control import ControlState
    from chanamq_amd.engine.golden import GoldenDataPlane
    for cls in (ControlState, GoldenDataPlane):
        with pytest.raises(ValueError, match="dead_letter"):
            cls(x_death=True)
        assert cls(dead_letter=True, x_death=True).x_death and not cls(dead_letter=True).x_death


def test_config_key():
    from chanamq_amd.utils.config import Config
    c = Config.load([], {}, env=False)
    c.set("chana.mq.gpu.dead-letter", True)
    assert "x_death" not in c.gpu_config()[0]
    c.set("chana.mq.gpu.dead-letter-x-death", True)
    plane, broker = c.gpu_config()
    assert plane["x_death"] is True and broker["x_death"] is True
    c.set("chana.mq.gpu.dead-letter", False)
    with pytest.raises(ValueError, match="dead-letter"):
        c.gpu_config()
