"""The opt-in features of the GPU path, layer by layer: which combinations construct, what
``gpu_config()`` hands to plane and broker, what reaches the engine's cfg dict, which statistics
the broker shows.  The rules are written out here, not read from the table under test
(chanamq_amd/engine/features.py).  No GPU."""

import itertools
import os

import pytest

from dp_scenarios import SCENARIOS, run
from gpu_cfg import CFG

NAMES = ("headers_match", "queue_limits", "queue_limit_bytes", "priority_queues", "dead_letter", "x_death",
         "alternate_exchange")
HOCON = {"headers_match": "headers-match", "queue_limits": "queue-limits", "queue_limit_bytes": "queue-limit-bytes",
         "priority_queues": "priority-queues", "dead_letter": "dead-letter", "x_death": "dead-letter-x-death",
         "alternate_exchange": "alternate-exchange"}
ALL = [dict(zip(NAMES, bits)) for bits in itertools.product((False, True), repeat=len(NAMES))]
OFF, ON = ALL[0], ALL[-1]


def invalid(f, world=1):
    return bool((f["x_death"] and not f["dead_letter"]) or (f["queue_limit_bytes"] and not f["queue_limits"])
                or ((f["dead_letter"] or f["priority_queues"]) and world > 1))


VALID = [f for f in ALL if not invalid(f)]
SMALL = dict(c_max=CFG["c_max"], chpc=CFG["chpc"], q_max=CFG["q_max"], x_max=CFG["x_max"], cons_max=CFG["cons_max"],
             default_queue_capacity=CFG["default_queue_capacity"])


def only(*names):
    return dict(OFF, **dict.fromkeys(names, True))


def golden(flags, **kw):
    from chanamq_amd.engine.golden import GoldenDataPlane
    return GoldenDataPlane(ucap=CFG["ucap"], carry_cap=CFG["carry_cap"], **SMALL, **kw, **flags)


def test_the_combinations():
    assert len(ALL) == 128 and len(VALID) == 72
    assert sum(not invalid(f, 2) for f in ALL) == 12


# ------------------------------------------------------------------ validation
def _control(flags, world):
    from chanamq_amd.engine.control import ControlState
    return ControlState(world=world, **SMALL, **flags)


def _golden(flags, world):
    return golden(flags, world=world, xfer_desc_max=16, xfer_bytes=4096)


def _features(flags, world):
    from chanamq_amd.engine.features import Features
    f = Features(**flags)
    assert f.validate(world) is f
    return f


@pytest.mark.parametrize("world", [1, 2])
@pytest.mark.parametrize("make", [_features, _control, _golden])
def test_validation(make, world):
    from chanamq_amd.engine.features import Features
    for flags in ALL:
        if invalid(flags, world):
            with pytest.raises(ValueError):
                make(flags, world)
            continue
        p = make(flags, world)
        assert {n: getattr(p, n) for n in NAMES} == flags, flags
        if make is not _features:
            assert p.features == Features(**flags) and p.world == world


def test_take_pops_the_known_keywords_and_coerces():
    from chanamq_amd.engine.features import Features
    kw = dict(queue_limits=1, x_death=0, c_max=8)
    f = Features.take(kw)
    assert kw == {"c_max": 8}
    assert {n: getattr(f, n) for n in NAMES} == only("queue_limits")


def test_control_state_refuses_unknown_keywords():
    from chanamq_amd.engine.control import ControlState
    with pytest.raises(TypeError):
        ControlState(queue_limit=True)
    with pytest.raises(TypeError):
        golden(OFF, no_such_option=1)


# ------------------------------------------------------------------ gpu_config()
def _gpu_config(tmp_path, lines, single=True):
    from chanamq_amd.utils.config import Config
    f = tmp_path / "f.conf"
    f.write_text("".join(f"chana.mq.gpu.{k} = {v}\n" for k, v in lines.items()))
    return Config.load([str(f)], {}).gpu_config(single=single)


PLANE_EXTRA = {"headers_match": dict(hb_max=1024, hp_max=4096), "dead_letter": dict(dead_max=1024, dead_bytes=8 << 20)}


@pytest.mark.parametrize("single", [True, False])
@pytest.mark.parametrize("on", [(), *((n,) for n in NAMES if n not in ("queue_limit_bytes", "x_death")),
                                ("queue_limits", "queue_limit_bytes"), ("dead_letter", "x_death"), NAMES],
                         ids=lambda on: "+".join(on) or "none")
def test_gpu_config_dicts(tmp_path, on, single):
    base_plane, base_broker = _gpu_config(tmp_path, {}, single)
    assert not set(base_plane) & (set(NAMES) | {"hb_max", "hp_max", "dead_max", "dead_bytes"})
    assert {n: base_broker[n] for n in NAMES} == OFF
    plane, broker = _gpu_config(tmp_path, {HOCON[n]: "true" for n in on}, single)
    want = dict(base_plane, **dict.fromkeys(on, True))
    for n in on:
        want.update(PLANE_EXTRA.get(n, {}))
    assert plane == want
    assert broker == dict(base_broker, **only(*on))
    assert all(plane[n] is True for n in on) and all(type(broker[n]) is bool for n in NAMES)


def test_gpu_config_sub_parameters(tmp_path):
    sizes = {"headers-bindings": 10, "headers-pairs": 7, "dead-max": 5, "dead-bytes": 4096}
    plane, _ = _gpu_config(tmp_path, sizes)   # (they ride with their feature: off, they are not read)
    assert not set(plane) & {"hb_max", "hp_max", "dead_max", "dead_bytes"}
    plane, _ = _gpu_config(tmp_path, dict(sizes, **{"headers-match": "on", "dead-letter": "on"}))
    assert (plane["hb_max"], plane["hp_max"], plane["dead_max"], plane["dead_bytes"]) == (10, 7, 5, 4096)
    plane, _ = _gpu_config(tmp_path, {"headers-match": "on", "headers-bindings": 10})
    assert (plane["hb_max"], plane["hp_max"]) == (10, 4096)   # (conf/reference.conf's headers-pairs)
    from chanamq_amd.utils.config import Config
    bare = Config()   # without the reference file: the defaults in the code, four pairs a binding
    bare.set("chana.mq.amqp.connection.frame-max", 131072)
    bare.set("chana.mq.gpu.headers-match", True)
    bare.set("chana.mq.gpu.dead-letter", True)
    plane, _ = bare.gpu_config()
    assert (plane["hb_max"], plane["hp_max"], plane["dead_max"], plane["dead_bytes"]) == (1024, 4096, 1024, 8 << 20)
    bare.set("chana.mq.gpu.headers-bindings", 10)
    assert bare.gpu_config()[0]["hp_max"] == 40


def test_gpu_config_names_the_keys_of_a_missing_requirement(tmp_path):
    with pytest.raises(ValueError, match=r"^chana\.mq\.gpu\.queue-limit-bytes needs chana\.mq\.gpu\.queue-limits$"):
        _gpu_config(tmp_path, {"queue-limit-bytes": "true"})
    with pytest.raises(ValueError, match=r"^chana\.mq\.gpu\.dead-letter-x-death needs chana\.mq\.gpu\.dead-letter$"):
        _gpu_config(tmp_path, {"dead-letter-x-death": "true"})
    with pytest.raises(ValueError, match="queue-limit-bytes"):   # both missing: the byte limit's speaks first
        _gpu_config(tmp_path, {"dead-letter-x-death": "true", "queue-limit-bytes": "true"})


# ------------------------------------------------------------------ the engine's cfg dict
class _Stop(Exception):
    pass


@pytest.fixture
def engine_cfgs(monkeypatch):
    """``GpuDataPlane`` over a stand-in extension whose Engine records its cfg and stops."""
    from chanamq_amd.engine import dataplane
    seen = []

    class Engine:
        def __init__(self, cfg):
            seen.append(dict(cfg))
            raise _Stop

    monkeypatch.setattr(dataplane.ops, "load", lambda: type("mod", (), {"Engine": Engine}))
    return seen


def test_engine_cfg(engine_cfgs):
    from chanamq_amd.engine.dataplane import GpuDataPlane
    for flags in VALID:
        with pytest.raises(_Stop):
            GpuDataPlane(**CFG, **flags)
        cfg = engine_cfgs.pop()
        want = {n: int(flags[n]) for n in ("queue_limits", "dead_letter", "x_death", "alternate_exchange")}
        want.update({n: 1 for n in ("queue_limit_bytes", "priority_queues") if flags[n]})
        assert {k: v for k, v in cfg.items() if k in NAMES} == want, flags
        assert all(type(cfg[n]) is int for n in want)
        assert {k: cfg[k] for k in CFG if k != "default_queue_capacity"} == \
            {k: v for k, v in CFG.items() if k != "default_queue_capacity"}
    with pytest.raises(_Stop):   # sizes and unknown keywords are the engine's to judge
        GpuDataPlane(headers_match=True, hb_max=10, hp_max=40, dead_max=5, no_such_option=3, **CFG)
    cfg = engine_cfgs.pop()
    assert (cfg["hb_max"], cfg["hp_max"], cfg["dead_max"], cfg["no_such_option"]) == (10, 40, 5, 3)
    assert "headers_match" not in cfg


@pytest.mark.parametrize("world", [1, 2])
def test_invalid_combinations_never_reach_the_engine(engine_cfgs, world):
    from chanamq_amd.engine.dataplane import GpuDataPlane
    for flags in ALL:
        if invalid(flags, world):
            with pytest.raises(ValueError):
                GpuDataPlane(world=world, **CFG, **flags)
    assert engine_cfgs == []


# ------------------------------------------------------------------ GpuBroker over a golden plane
DL_STATS = ("dl_expired", "dl_maxlen", "dl_rejected", "dl_unrouted", "dl_dropped", "dl_pending")
STATS = {"queue_limits": ("maxlen_dropped", "maxlen_rejected"), "dead_letter": DL_STATS, "x_death": ("dl_cycle",),
         "alternate_exchange": ("alt_routed",)}


def broker(plane, **kw):
    from chanamq_amd.server.gpu_broker import GpuBroker
    b = GpuBroker(plane, io="python", **kw)
    os.close(b._wake_r), os.close(b._wake_w), b._sel.close()   # (never started: nothing else is open)
    return b


def test_broker_statistics_keys():
    from chanamq_amd.server.gpu_broker import GpuBroker
    assert GpuBroker.DL_STATS == DL_STATS
    base = ["steps", "published", "delivered", "connections"]
    assert list(broker(golden(OFF)).stats) == base
    assert list(broker(golden(ON)).stats) == base   # a flag may be off over a plane that has it on
    for flags in VALID:
        b = broker(golden(flags), **flags)
        assert {n: getattr(b, n) for n in NAMES} == flags
        want = base + [s for n in NAMES if flags[n] for s in STATS.get(n, ())]
        assert list(b.stats) == want and not any(b.stats.values()), flags


def test_broker_statistics_follow_the_step_counters():
    b = broker(golden(ON), **ON)
    cnt = dict(n_pubs=1, n_maxlen_dropped=2, n_maxlen_rejected=3, n_dl_expired=4, n_dl_maxlen=5, n_dl_rejected=6,
               n_dl_unrouted=7, n_dl_dropped=8, n_dl_pending=9, n_dl_cycle=10, n_alt=11)
    for _ in range(2):
        b._after_step([], [], [], cnt, False, False)
    want = dict(steps=2, published=2, delivered=0, connections=0, maxlen_dropped=4, maxlen_rejected=6, dl_expired=8,
                dl_maxlen=10, dl_rejected=12, dl_unrouted=14, dl_dropped=16, dl_pending=9, dl_cycle=20, alt_routed=22)
    assert b.stats == want   # (dl_pending is the device's count of now, not a sum)
    b = broker(golden(ON))
    b._after_step([], [], [], cnt, False, False)
    assert b.stats == dict(steps=1, published=1, delivered=0, connections=0)


@pytest.mark.parametrize("name", NAMES)
def test_broker_flag_needs_its_plane(name):
    need = {"queue_limit_bytes": "queue_limits", "x_death": "dead_letter"}.get(name)
    flags = only(name, *([need] if need else []))
    with pytest.raises(ValueError, match=f"^{name}=True needs a data plane built with {name}=True$"):
        broker(golden(only(*([need] if need else []))), **flags)
    if need:
        with pytest.raises(ValueError, match=f"^{name}=True needs {need}=True$"):
            broker(golden(ON), **only(name))
    assert getattr(broker(golden(ON), **flags), name) is True


@pytest.mark.parametrize("name", ["dead_letter", "priority_queues"])
def test_broker_flag_not_served_on_a_sharded_node(name):
    with pytest.raises(ValueError, match=f"^{name}=True is not served on a sharded node$"):
        broker(golden(ON), node=object(), **only(name))


def test_broker_refuses_unknown_keywords():
    with pytest.raises(TypeError):
        broker(golden(OFF), queue_limit=True)


# ------------------------------------------------------------------ the golden model is flag-transparent
MATRIX_SCENARIOS = ("nack_requeue", "basic_get", "ttl", "confirm_mandatory")


@pytest.mark.parametrize("name", MATRIX_SCENARIOS)
def test_golden_scenarios_do_not_depend_on_the_flags(name):
    """The scenarios tests/test_gpu_feature_matrix.py runs declare no feature argument: the golden
    plane built with any valid combination answers as the all-off plane does."""
    def outputs(flags):
        g = golden(flags)
        return run(g, SCENARIOS[name](g), now_step_ms=3000)
    want = outputs(OFF)
    for flags in VALID:
        assert outputs(flags) == want, flags
