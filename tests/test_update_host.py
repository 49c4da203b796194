"""Host test of the update driver (limo-velo_amd/csrc/lv_update.hpp) and the knob table (lv_knobs.hpp): which launches an
iterated update enqueues on each route, with which arguments, what every entry point refuses and when, and what a failure at
any point of any sequence leaves behind.

tests/emu/update_emu.cpp compiles the product's own UpdateDriver (with ResidentFilter and RankExchange) with g++ against the
stand-in tests/emu/hip/hip_runtime.h and fake launches that log their arguments and write a toy posterior.  Each scenario runs as
its own process, once in a plain build and once under AddressSanitizer + UndefinedBehaviorSanitizer.  The failures cannot be
reached on a GPU (nobody may provoke a HIP error there); the routes' results on a real MI355X are tests/test_gpu_update_routes.py.

split_api holds the failed-begin case: a begin that fails must leave in_update false.  Before the driver moved into its header,
lv_update_begin set the flag first and never cleared it, so that check fails on the commit before.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")
BUILD_DIR = os.path.join(EMU_DIR, "_build")
CSRC = os.path.join(ROOT, "limo-velo_amd", "csrc")
SOURCES = [os.path.join(EMU_DIR, "update_emu.cpp"), os.path.join(EMU_DIR, "hip", "hip_runtime.h")] + \
          [os.path.join(CSRC, h) for h in ("lv_update.hpp", "lv_knobs.hpp", "lv_filter.hpp", "lv_exchange.hpp", "lv_observe.hpp", "lv_common.hpp",
                                           "lv_device.hpp")] + [os.path.join(ROOT, "include", "limovelo_hip.h")]
BUILDS = {"plain": [], "asan": ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]}
SCENARIOS = ["fused_by_value", "three_kernel_by_value", "route_table", "iterate", "split_api", "failures_by_value", "failures_correct",
             "update_end", "peer_failure", "update_no_map", "correct", "buffers", "knobs", "random1", "random2", "random3"]


@pytest.fixture(scope="module")
def emu_bins():
    os.makedirs(BUILD_DIR, exist_ok=True)
    bins = {b: os.path.join(BUILD_DIR, "update_emu_" + b) for b in BUILDS}
    stale = [b for b, exe in bins.items()
             if not os.path.exists(exe) or any(os.path.getmtime(s) > os.path.getmtime(exe) for s in SOURCES)]
    procs = [(b, subprocess.Popen(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-I" + EMU_DIR, *BUILDS[b],
                                   "-o", bins[b], SOURCES[0]], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
             for b in stale]
    for b, p in procs:
        out, _ = p.communicate()
        assert p.returncode == 0, f"{b} build failed:\n{out}"
        assert "warning" not in out, out
    return bins


@pytest.mark.parametrize("build", list(BUILDS))
@pytest.mark.parametrize("scenario", SCENARIOS)
def test_update_scenario(emu_bins, scenario, build):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([emu_bins[build], scenario], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, f"{scenario} ({build}) exited {r.returncode}:\n{r.stderr[-4000:]}"
    assert "runtime error" not in r.stderr, r.stderr[-4000:]
    assert r.stdout.strip() == "ok " + scenario
