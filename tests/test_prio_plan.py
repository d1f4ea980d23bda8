"""The priority walk and the split of V (csrc/kernels/prio_plan.h: what k_prio_lane and
k_prio_dispatch run on the device) as a stand-alone program under the address and
undefined-behaviour sanitizers, never loaded into Python: its own cases, and -- through a pipe --
generated property lists cut at every byte, whose priority must equal the Python codec's reading
(a list the codec cannot decode has no properties) and the golden model's walk."""

import os
import random
import shutil
import subprocess

import pytest

from chanamq_amd.engine import prio
from chanamq_amd.protocol.codec import decode_properties, encode_properties

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = os.path.join(ROOT, "csrc", "kernels")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ is needed to build tests/native/prio_plan_test.cpp")
    out = str(tmp_path_factory.mktemp("prio") / "prio_plan_test")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan", f"-I{KERNELS}",
                    os.path.join(ROOT, "tests", "native", "prio_plan_test.cpp"), "-o", out], check=True)
    return out


def test_plan_under_sanitizers(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "ok" and not r.stderr.strip(), r.stdout + r.stderr


def by_codec(raw):
    """The priority as the Python codec reads the list: 0 when absent or when it cannot be decoded."""
    try:
        props, _ = decode_properties(raw)
    except Exception:   # noqa: BLE001 - a list cut short
        return 0
    return props.get("priority") or 0


def _lists():
    rng = random.Random(20241021)
    ahead = [{}, {"content_type": "text/plain"}, {"content_encoding": "gzip"}, {"headers": {"k": "v", "n": 7, "t": {"a": 1}}},
             {"delivery_mode": 2}, {"content_type": "a", "content_encoding": "", "headers": {}, "delivery_mode": 1}]
    behind = [{}, {"correlation_id": "c" * 40}, {"expiration": "1500", "timestamp": 1_700_000_000},
              {"reply_to": "r", "message_id": "m", "type": "t", "user_id": "u", "app_id": "a", "cluster_id": "x"}]
    out = []
    for a in ahead:
        for b in behind:
            for pr in (None, 0, 1, 15, 16, 255):
                p = dict(a, **b)
                if pr is not None:
                    p["priority"] = pr
                out.append(encode_properties(p))
    for _ in range(40):   # random subsets of all fourteen
        p = {}
        for name, val in (("content_type", "ct"), ("content_encoding", "ce"), ("headers", {"h": rng.randrange(99)}),
                          ("delivery_mode", rng.choice((1, 2))), ("priority", rng.randrange(256)), ("correlation_id", "co"),
                          ("reply_to", "rt"), ("expiration", str(rng.randrange(10 ** 6))), ("message_id", "mi" * rng.randrange(9)),
                          ("timestamp", 1_700_000_000 + rng.randrange(999)), ("type", "ty"), ("user_id", "us"), ("app_id", "ap"),
                          ("cluster_id", "cl")):
            if rng.random() < 0.5:
                p[name] = val
        out.append(encode_properties(p))
    return out


def test_walk_equals_the_codec_at_every_truncation_point(exe):
    cases = []
    for raw in _lists():
        cases += [raw[:n] for n in range(len(raw) + 1)]            # every truncation point, the whole list last
        cases.append(bytes([raw[0], raw[1] | 1, 0, 0]) + raw[2:])   # a continuation word without fields
    text = "".join((c.hex() or "-") + "\n" for c in cases)
    r = subprocess.run([exe, "pipe"], input=text, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and not r.stderr.strip(), r.stderr[-2000:]
    got = [int(x) for x in r.stdout.split()]
    assert len(got) == len(cases) > 5000
    seen = set()
    for c, g in zip(cases, got):
        assert g == by_codec(c) == prio.prio_of_props(c), f"props {c.hex()}"
        seen.add(g)
    assert {0, 1, 15, 16, 255} <= seen


def test_split_piece_is_the_brute_force_one():
    rng = random.Random(7)
    for _ in range(300):
        counts = [rng.randrange(5) for _ in range(rng.randrange(1, 17))]
        v = [(lane, k) for lane, n in enumerate(counts) for k in range(n)]
        off = rng.randrange(len(v) + 1)
        cnt = rng.randrange(len(v) - off + 1)
        got = [(lane, pos + k) for lane, pos, n in prio.split_piece(counts, off, cnt) for k in range(n)]
        assert got == v[off:off + cnt]
    assert [prio.lane_of(p, 3) for p in (0, 1, 3, 4, 255)] == [3, 2, 0, 0, 0]
