"""bench.py --dump-outputs: the arrays written for a step do not depend on how the step
interleaved its publishers (unordered by design), and do depend on what was delivered."""

import numpy as np

import bench
from chanamq_amd.engine.layout import CONN_OUT
from chanamq_amd.protocol.codec import Method, render_command


class _Eng:
    def counters(self, parity):
        return {"n_pubs": 4, "n_deliv": 4}


class _Plane:
    """Stands in for a finished step: ``host_egress`` hands back its wire bytes."""

    def __init__(self, per_conn):
        self.eng = _Eng()
        co = np.zeros(8, CONN_OUT)
        buf = b""
        for conn, cmds in per_conn.items():
            wire = b"".join(render_command(1, Method("basic.deliver", consumer_tag=f"c{conn}", delivery_tag=tag,
                                                     exchange="x", routing_key=key), {"delivery_mode": 1}, body)
                            for tag, (key, body) in enumerate(cmds, 7))
            co[conn] = (len(buf), len(wire))
            buf += wire
        self._eg = (np.frombuffer(buf, np.uint8), co)

    def host_egress(self, ticket):
        return self._eg


def _dump(tmp_path, name, per_conn):
    d = tmp_path / name
    bench.dump_outputs(_Plane(per_conn), (0, 0, 0.0, 0), str(d))
    return {f.name: np.load(f) for f in sorted(d.iterdir())}


def test_dump_is_canonical_across_publisher_interleaving(tmp_path):
    a, b = ("k.a", b"A" * 300), ("k.b", b"B" * 200)
    c, e = ("k.c", b"C" * 100), ("k.e", b"")
    one = _dump(tmp_path, "one", {3: [a, b], 5: [c, e]})
    two = _dump(tmp_path, "two", {3: [b, a], 5: [e, c]})
    assert sorted(one) == ["counters.npy", "deliveries.npy", "delivery_tags.npy", "egress_wire.npy"]
    for k in one:
        assert one[k].dtype in (np.float32, np.float64)
        assert np.array_equal(one[k], two[k]), k
    assert one["deliveries.npy"].shape == (4, 4) and list(one["deliveries.npy"][:, 0]) == [3, 3, 5, 5]
    assert one["delivery_tags.npy"].tolist() == [[3, 7, 8], [5, 7, 8]]
    # a changed body byte, or a message delivered to another consumer, shows
    bad = _dump(tmp_path, "bad", {3: [a, ("k.b", b"B" * 199 + b"b")], 5: [c, e]})
    assert not np.array_equal(one["deliveries.npy"], bad["deliveries.npy"])
    assert not np.array_equal(one["egress_wire.npy"], bad["egress_wire.npy"])
    moved = _dump(tmp_path, "moved", {3: [a], 5: [b, c, e]})
    assert not np.array_equal(one["deliveries.npy"], moved["deliveries.npy"])


def test_plain_run_skips_what_full_adds():
    """The checked extra steps and the soak belong to ``--full``; an explicit ``--soak-s``
    is honoured either way."""
    plain = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "3"])
    assert (plain.steps, plain.warmup, plain.full, plain.dump_outputs) == (7, 3, False, None)
    assert plain.verify_steps == 0 and plain.soak_s == 0.0
    full = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "3", "--full"])
    assert full.verify_steps == 2 and full.soak_s == 2.0
    assert bench.parse_args(["--full", "--egress-ref", "0"]).verify_steps == 0
    assert bench.parse_args(["--full", "--soak-s", "0"]).soak_s == 0.0
    assert bench.parse_args(["--soak-s", "1.5"]).soak_s == 1.5
    assert bench.parse_args(["--dump-outputs", "d"]).dump_outputs == "d"
