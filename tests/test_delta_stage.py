"""Host-only checks of the engine's sources: the deferred control-write stager under the
address and undefined-behaviour sanitizers (a stand-alone program, never loaded into Python),
and the extension's rebuild list against what engine.hip really includes."""

import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = os.path.join(ROOT, "csrc", "kernels")


def test_delta_stage_under_sanitizers(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ is needed to build tests/native/delta_stage_test.cpp")
    exe = str(tmp_path / "delta_stage_test")
    # (the sanitizer runtimes linked statically: the program runs as it is, whatever else
    # the environment loads into processes)
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan", f"-I{KERNELS}",
                    os.path.join(ROOT, "tests", "native", "delta_stage_test.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "ok" and not r.stderr.strip(), r.stdout + r.stderr


def test_sources_cover_engine_includes():
    """Every file engine.hip reaches through #include "..." inside csrc/kernels is hashed by
    ops._stale(): a change to any of them rebuilds the extension."""
    from chanamq_amd import ops

    seen, todo = set(), ["engine.hip"]
    while todo:
        name = todo.pop()
        if name in seen:
            continue
        seen.add(name)
        with open(os.path.join(KERNELS, name)) as f:
            for inc in re.findall(r'^\s*#\s*include\s+"([^"]+)"', f.read(), re.M):
                if os.path.exists(os.path.join(KERNELS, inc)):
                    todo.append(inc)
    assert "delta_stage.h" in seen and "dataplane.hip" in seen
    assert seen <= set(ops.SOURCES), sorted(seen - set(ops.SOURCES))
