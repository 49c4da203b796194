"""Host test of lv_observe's side of the resident filter (limo-velo_amd/csrc/lv_filter.hpp: ResidentFilter::observe) and of its
argument rules (limo-velo_amd/csrc/lv_observe.hpp).

tests/emu/observe_emu.cpp compiles the product's own ResidentFilter with g++ against the stand-in tests/emu/hip/hip_runtime.h
(synchronous, logged calls; counted allocations) and fake launches, and drives observe from every place the filter can be: what
is enqueued, in which order, and where the filter is afterwards.  Each scenario runs as its own process, once in a plain build
and once under AddressSanitizer + UndefinedBehaviorSanitizer.  The GPU side of the same paths is tests/test_gpu_observe.py."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")
BUILD_DIR = os.path.join(EMU_DIR, "_build")
CSRC = os.path.join(ROOT, "limo-velo_amd", "csrc")
SOURCES = [os.path.join(EMU_DIR, "observe_emu.cpp"), os.path.join(EMU_DIR, "hip", "hip_runtime.h"),
           os.path.join(CSRC, "lv_filter.hpp"), os.path.join(CSRC, "lv_observe.hpp"), os.path.join(CSRC, "lv_common.hpp"),
           os.path.join(CSRC, "lv_device.hpp"), os.path.join(ROOT, "include", "limovelo_hip.h")]
BUILDS = {"plain": [], "asan": ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]}
SCENARIOS = ["from_host", "from_device_queued", "from_kf", "from_kf_queued", "from_copied", "unset", "observe_predict_observe",
             "then_correct", "rejections", "defaults"]


@pytest.fixture(scope="module")
def emu_bins():
    os.makedirs(BUILD_DIR, exist_ok=True)
    bins = {b: os.path.join(BUILD_DIR, "observe_emu_" + b) for b in BUILDS}
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
def test_observe_scenario(emu_bins, scenario, build):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([emu_bins[build], scenario], capture_output=True, text=True, timeout=60, env=env)
    assert r.returncode == 0, f"{scenario} ({build}) exited {r.returncode}:\n{r.stderr[-4000:]}"
    assert "runtime error" not in r.stderr, r.stderr[-4000:]
    assert r.stdout.strip() == "ok " + scenario
