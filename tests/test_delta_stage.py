"""Host-only checks of the engine's sources: the deferred control-write stager under the
address and undefined-behaviour sanitizers, the SDMA copy plan, the exchange worker and the
side-operation mailbox under those and the thread sanitizer (stand-alone programs, never
loaded into Python), and the extension's rebuild list against what engine.hip really includes."""

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


ENGINE_HOST_TEST = os.path.join(ROOT, "tests", "native", "engine_host_test.cpp")


def test_engine_host_logic_under_asan_ubsan(tmp_path):
    """The SDMA copy plan, the exchange worker and the side-operation mailbox (sdma_plan.h,
    xchg_worker.h, side_box.h) as a stand-alone program under ASan + UBSan."""
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ is needed to build tests/native/engine_host_test.cpp")
    exe = str(tmp_path / "engine_host_test")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan", "-pthread", f"-I{KERNELS}", ENGINE_HOST_TEST, "-o", exe],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "ok" and not r.stderr.strip(), r.stdout + r.stderr


def test_engine_host_logic_under_tsan(tmp_path):
    """The same program under ThreadSanitizer, built with the ROCm LLVM clang++ as
    scripts/host_sanitize.sh does: gcc 11's libtsan does not intercept the timed
    condition-variable wait the side box uses and reports a false double lock there."""
    cxx = "/opt/rocm/lib/llvm/bin/clang++"
    if not os.path.exists(cxx):
        pytest.fail(cxx + " is needed to build tests/native/engine_host_test.cpp with -fsanitize=thread")
    exe = str(tmp_path / "engine_host_tsan")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=thread", "-pthread", f"-I{KERNELS}", ENGINE_HOST_TEST,
                    "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, TSAN_OPTIONS="halt_on_error=1:second_deadlock_stack=1"))
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


def test_every_kernel_is_launched():
    """Every __global__ kernel defined under csrc/kernels is named at least once outside its
    own definition (comments aside) in engine.hip or in a HIP / C++ source under bench/: a
    kernel nothing launches is dead code that every build still compiles."""
    definition = r"__global__\b[^;{]*?\bvoid\s+(\w+)\s*\("

    def code(path):
        with open(path) as f:
            return re.sub(r"//[^\n]*|/\*.*?\*/", "", f.read(), flags=re.S)

    defs = set()
    for name in os.listdir(KERNELS):
        defs.update(re.findall(definition, code(os.path.join(KERNELS, name))))
    assert len(defs) > 40, sorted(defs)   # (the pattern still finds the kernels)
    users = [os.path.join(KERNELS, "engine.hip")]
    for dirpath, _, files in os.walk(os.path.join(ROOT, "bench")):
        users += [os.path.join(dirpath, f) for f in files if f.endswith((".hip", ".cpp", ".h"))]
    text = "\n".join(re.sub(definition, "", code(path)) for path in users)
    dead = sorted(k for k in defs if not re.search(r"\b%s\b" % k, text))
    assert not dead, dead
