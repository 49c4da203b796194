"""Host test of the background map rebuild (limo-velo_amd/csrc/lv_rebuild.hpp): its state machine, journal, locking and failure exits.

tests/emu/rebuild_emu.cpp compiles the product's own MapRebuild template with g++ against the stand-in tests/emu/hip/hip_runtime.h
(synchronous, logged streams and events; counted allocations) and a fake store whose operations the scenario holds at a gate or
makes fail on the worker thread.  Each scenario runs as its own process, once in a plain build and once under ThreadSanitizer.
The GPU side of the same machinery is tests/test_gpu_map_async.py.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")
BUILD_DIR = os.path.join(EMU_DIR, "_build")
SOURCES = [os.path.join(EMU_DIR, "rebuild_emu.cpp"), os.path.join(EMU_DIR, "hip", "hip_runtime.h"),
           os.path.join(ROOT, "limo-velo_amd", "csrc", "lv_rebuild.hpp"), os.path.join(ROOT, "limo-velo_amd", "csrc", "lv_common.hpp"),
           os.path.join(ROOT, "include", "limovelo_hip.h")]
BUILDS = {"plain": [], "tsan": ["-fsanitize=thread", "-static-libtsan"]}
SCENARIOS = ["full_cycle", "replay_in_order", "journal_bound", "adoption_race", "cancel", "worker_failure", "outgrow",
             "arena_exhausted", "stream_order", "status_wait"]
# what a scenario must say on stderr (the product's own lines)
STDERR = {"journal_bound": ["background map rebuild cannot keep up (3 journaled operations)"],
          "worker_failure": ["background map rebuild failed (reserve:", "background map rebuild failed (wait for the snapshot:",
                             "background map rebuild failed (rebuild:", "background map rebuild failed (replay of a journaled map operation:"]}


@pytest.fixture(scope="module")
def emu_bins():
    os.makedirs(BUILD_DIR, exist_ok=True)
    bins = {b: os.path.join(BUILD_DIR, "rebuild_emu_" + b) for b in BUILDS}
    stale = [b for b, exe in bins.items()
             if not os.path.exists(exe) or any(os.path.getmtime(s) > os.path.getmtime(exe) for s in SOURCES)]
    procs = [(b, subprocess.Popen(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-I" + EMU_DIR, *BUILDS[b], "-o", bins[b], SOURCES[0], "-pthread"],
                                  stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)) for b in stale]
    for b, p in procs:
        out, _ = p.communicate()
        assert p.returncode == 0, f"{b} build failed:\n{out}"
    return bins


@pytest.mark.parametrize("build", list(BUILDS))
@pytest.mark.parametrize("scenario", SCENARIOS)
def test_rebuild_scenario(emu_bins, scenario, build):
    env = dict(os.environ, TSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([emu_bins[build], scenario], capture_output=True, text=True, timeout=60, env=env)
    assert r.returncode == 0, f"{scenario} ({build}) exited {r.returncode}:\n{r.stderr[-4000:]}"
    assert "ThreadSanitizer" not in r.stderr, r.stderr[-4000:]
    assert r.stdout.strip() == "ok " + scenario
    for line in STDERR.get(scenario, []):
        assert line in r.stderr, (line, r.stderr)
    if scenario not in STDERR:
        assert "[limovelo_hip]" not in r.stderr, r.stderr
