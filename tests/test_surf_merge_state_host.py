"""Host test of lv_surf_merge's state rules (limo-velo_amd/csrc/lv_volumes.hpp: VolumeTools::surf_merge, its row of the stale
table): LV_ESTATE before lv_tsdf_configure, then the resolution ratio against the volume (LV_EINVAL, nothing marked); once the
arguments hold a built mesh goes stale and the surface rays' packed states are marked not packed, whatever the store call returns;
the colour layer, the occupancy grid and everything built from it are never touched, and no grid is asked for; a submap whose box
cannot meet the volume gives LV_OK, zero stats and no store call.

tests/emu/surf_merge_state_emu.cpp compiles the product's own lv_volumes.hpp and tool headers with g++ against the stand-in
tests/emu/hip/hip_runtime.h and its own stand-ins for the stores' member functions, in the manner of
tests/emu/surf_occ_state_emu.cpp (tests/emu/volumes_emu.cpp stays as it is and knows nothing of this call).  Each scenario runs as
its own process, once in a plain build and once under AddressSanitizer + UndefinedBehaviorSanitizer.  The GPU side of the same
rules is tests/test_gpu_surf_merge.py."""
import glob
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")
BUILD_DIR = os.path.join(EMU_DIR, "_build")
CSRC = os.path.join(ROOT, "limo-velo_amd", "csrc")
SOURCES = [os.path.join(EMU_DIR, "surf_merge_state_emu.cpp"), os.path.join(EMU_DIR, "hip", "hip_runtime.h"),
           os.path.join(ROOT, "include", "limovelo_hip.h"), *sorted(glob.glob(os.path.join(CSRC, "*.hpp")))]
BUILDS = {"plain": [], "asan": ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]}
SCENARIOS = ["order", "marks", "empty_box"]


@pytest.fixture(scope="module")
def emu_bins():
    os.makedirs(BUILD_DIR, exist_ok=True)
    bins = {b: os.path.join(BUILD_DIR, "surf_merge_state_emu_" + b) for b in BUILDS}
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
def test_surf_merge_state_scenario(emu_bins, scenario, build):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([emu_bins[build], scenario], capture_output=True, text=True, timeout=60, env=env)
    assert r.returncode == 0, f"{scenario} ({build}) exited {r.returncode}:\n{r.stderr[-4000:]}"
    assert "runtime error" not in r.stderr, r.stderr[-4000:]
    assert r.stdout.strip() == "ok " + scenario
