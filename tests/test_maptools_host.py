"""Host test of the map tools' call order (limo-velo_amd/csrc/lv_maptools.hpp: MapSide, MapTools): how lv_map_remove_dynamic,
lv_map_normals, lv_map_remove_outliers, lv_map_cluster, lv_map_remove_clusters, lv_map_planes, lv_map_paint and the three queries
order themselves against an insert in flight and a background rebuild, what each judges before the map is looked at, when it
zeroes its outputs, what a removal journals and what the worker replays, what the map source of lv_elev_build, lv_ndt_build /
lv_ndt_add and lv_occ_mark hands on, and what is freed in which order.

tests/emu/maptools_emu.cpp compiles the product's own lv_maptools.hpp and tool headers with g++ against the stand-in
tests/emu/hip/hip_runtime.h (synchronous, logged calls; counted allocations), with stand-ins for the stores' member functions, the
tools' launches and the rebuild that log themselves with their telling arguments.  The expected logs are literals in that file.
Each scenario runs as its own process, once in a plain build and once under AddressSanitizer + UndefinedBehaviorSanitizer.  The GPU
side of the same calls is tests/test_gpu_map_*.py, tests/test_gpu_rules.py and tests/test_gpu_map_source_async.py."""
import glob
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")
BUILD_DIR = os.path.join(EMU_DIR, "_build")
CSRC = os.path.join(ROOT, "limo-velo_amd", "csrc")
SOURCES = [os.path.join(EMU_DIR, "maptools_emu.cpp"), os.path.join(EMU_DIR, "hip", "hip_runtime.h"),
           os.path.join(ROOT, "include", "limovelo_hip.h"), *sorted(glob.glob(os.path.join(CSRC, "*.hpp")))]
BUILDS = {"plain": [], "asan": ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]}
SCENARIOS = ["ready", "queries", "normals", "cluster", "planes", "paint", "remove_dynamic", "remove_outliers", "remove_clusters",
             "map_source", "release"]


@pytest.fixture(scope="module")
def emu_bins():
    os.makedirs(BUILD_DIR, exist_ok=True)
    bins = {b: os.path.join(BUILD_DIR, "maptools_emu_" + b) for b in BUILDS}
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
def test_maptools_scenario(emu_bins, scenario, build):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([emu_bins[build], scenario], capture_output=True, text=True, timeout=60, env=env)
    assert r.returncode == 0, f"{scenario} ({build}) exited {r.returncode}:\n{r.stderr[-4000:]}"
    assert "runtime error" not in r.stderr, r.stderr[-4000:]
    assert r.stdout.strip() == "ok " + scenario
