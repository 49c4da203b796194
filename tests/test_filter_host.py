"""Host test of the resident filter (limo-velo_amd/csrc/lv_filter.hpp): where x, P live, the prediction queue, and the HIP calls
each entry point makes on the filter's behalf.

tests/emu/filter_emu.cpp compiles the product's own ResidentFilter with g++ against the stand-in tests/emu/hip/hip_runtime.h
(synchronous, logged calls; counted allocations) and fake launches, and drives it as the update driver (lv_update.hpp; its own
host test is tests/test_update_host.py) and the entry points of lv_api.hip do.  Each scenario runs as its own process, once in a
plain build and once under AddressSanitizer + UndefinedBehaviorSanitizer.  The GPU side of the same paths is
tests/test_gpu_filter.py.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")
BUILD_DIR = os.path.join(EMU_DIR, "_build")
CSRC = os.path.join(ROOT, "limo-velo_amd", "csrc")
SOURCES = [os.path.join(EMU_DIR, "filter_emu.cpp"), os.path.join(EMU_DIR, "hip", "hip_runtime.h"),
           os.path.join(CSRC, "lv_filter.hpp"), os.path.join(CSRC, "lv_common.hpp"), os.path.join(CSRC, "lv_device.hpp"),
           os.path.join(ROOT, "include", "limovelo_hip.h")]
BUILDS = {"plain": [], "asan": ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]}
SCENARIOS = ["cycle", "set_get", "set_predict3_get", "queue_splits", "correct_predict_correct", "correct_update_predict_get",
             "set_predict_set", "mailbox_resync", "mailbox_unchecked", "mailbox_fault", "failures", "map_add_source",
             "random1", "random2", "random3"]


@pytest.fixture(scope="module")
def emu_bins():
    os.makedirs(BUILD_DIR, exist_ok=True)
    bins = {b: os.path.join(BUILD_DIR, "filter_emu_" + b) for b in BUILDS}
    stale = [b for b, exe in bins.items()
             if not os.path.exists(exe) or any(os.path.getmtime(s) > os.path.getmtime(exe) for s in SOURCES)]
    procs = [(b, subprocess.Popen(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-I" + EMU_DIR, *BUILDS[b],
                                   "-o", bins[b], SOURCES[0]], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
             for b in stale]
    for b, p in procs:
        out, _ = p.communicate()
        assert p.returncode == 0, f"{b} build failed:\n{out}"
    return bins


@pytest.mark.parametrize("build", list(BUILDS))
@pytest.mark.parametrize("scenario", SCENARIOS)
def test_filter_scenario(emu_bins, scenario, build):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([emu_bins[build], scenario], capture_output=True, text=True, timeout=60, env=env)
    assert r.returncode == 0, f"{scenario} ({build}) exited {r.returncode}:\n{r.stderr[-4000:]}"
    assert "runtime error" not in r.stderr, r.stderr[-4000:]
    assert r.stdout.strip() == "ok " + scenario
