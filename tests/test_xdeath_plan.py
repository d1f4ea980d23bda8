"""The x-death plan and writer (csrc/kernels/xdeath_plan.h: what the dead pass's size pass and write
pass both run on the device) as a stand-alone program under the address and undefined-behaviour
sanitizers, never loaded into Python: its own cases and mutated property lists, and -- through a
pipe -- the same inputs as the golden model's rewrite (chanamq_amd/engine/xdeath.py), whose
verdicts, bytes and banned names it must equal."""

import os
import random
import shutil
import subprocess

import pytest

from chanamq_amd.engine import xdeath
from chanamq_amd.protocol.codec import Typed, encode_properties

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = os.path.join(ROOT, "csrc", "kernels")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ is needed to build tests/native/xdeath_plan_test.cpp")
    out = str(tmp_path_factory.mktemp("xdeath") / "xdeath_plan_test")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan", f"-I{KERNELS}",
                    os.path.join(ROOT, "tests", "native", "xdeath_plan_test.cpp"), "-o", out], check=True)
    return out


def test_plan_under_sanitizers(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "ok" and not r.stderr.strip(), r.stdout + r.stderr


def _hex(b):
    return b.hex() or "-"


def _element(q, reason, count=Typed("l", 2)):
    e = {"count": count, "reason": reason, "queue": q, "time": Typed("T", 1_600_000_000), "exchange": "x",
         "routing-keys": ["k"]}
    return {k: v for k, v in e.items() if v is not None}


def _cases():
    rng = random.Random(20240607)
    both = {"content_type": "text/plain", "delivery_mode": 2, "correlation_id": "c", "timestamp": 1_700_000_000,
            "app_id": "app", "expiration": "1500"}
    arrays = [None, [], "text", [_element("work", "expired")], [_element("other", "maxlen"), _element("work", "rejected", 7)],
              [_element("a", "expired"), _element("b", "rejected"), _element("c", "expired"), _element("work", "expired", None)],
              [_element("a", "expired"), 5], [{"reason": "expired"}, _element("work", "maxlen", "many")],
              [_element(f"q{i}", "expired") for i in range(63)], [_element(f"q{i}", "expired") for i in range(64)]]
    lists = []
    for base in ({}, {"expiration": "9"}, both, {"headers": {"kind": "late"}}, dict(both, headers={"kind": "late", "n": 3})):
        for arr in arrays:
            p = dict(base)
            if arr is not None:
                p["headers"] = dict(p.get("headers") or {}, **{"x-death": arr})
            lists.append(encode_properties(p))
            if arr is not None:
                p["headers"] = dict(p["headers"], **{"x-first-death-queue": "first", "z": 1})
                p["headers"][b"x-death"] = [_element("dup", "expired")]
                lists.append(encode_properties(p))
    out = []
    for raw in lists:
        for reason in range(3):
            out.append((reason, b"work", b"in", b"k.1", 1_700_000_000 + reason, raw))
        for _ in range(20):   # mutated: a byte changed, a bit flipped, cut, a byte inserted
            m = bytearray(raw)
            for _ in range(rng.randint(1, 3)):
                if not m:
                    break
                at = rng.randrange(len(m))
                how = rng.randrange(4)
                if how == 0:
                    m[at] = rng.randrange(256)
                elif how == 1:
                    m[at] ^= 1 << rng.randrange(8)
                elif how == 2:
                    del m[at:]
                else:
                    m.insert(at, rng.randrange(256))
            out.append((rng.randrange(3), b"work", b"", b"", 5, bytes(m)))
    out.append((0, b"Q" * 255, b"X" * 255, b"k" * 255, 0, encode_properties({"expiration": "1"})))
    out.append((2, b"q", b"", b"", 1 << 40, b"\x00\x00"))
    return out


def test_plan_equals_the_golden_rewrite(exe):
    cases = _cases()
    text = "".join(f"{r} {_hex(q)} {_hex(ex)} {_hex(rk)} {t} {_hex(p)}\n" for r, q, ex, rk, t, p in cases)
    r = subprocess.run([exe, "pipe"], input=text, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and not r.stderr.strip(), r.stderr[-2000:]
    lines = r.stdout.split("\n")[:-1]
    assert len(lines) == len(cases) > 1000
    seen = set()
    for (reason, q, ex, rk, t, p), line in zip(cases, lines):
        st, out, names = xdeath.rewrite(p, q, reason, ex, rk, t)
        # (the native plan hands the source queue's own ban to its caller: the names of the old elements only)
        want_names = names[1:] if st == xdeath.REWRITE and reason != xdeath.REJECTED else names
        want = f"{st} {_hex(out) if st == xdeath.REWRITE else '-'} {','.join(_hex(n) for n in want_names) or '-'}"
        assert line == want, f"reason {reason} props {p.hex()}"
        seen.add(st)
    assert seen == {xdeath.VERBATIM, xdeath.REWRITE, xdeath.OVER}
