"""Host tests of the submap merge: the rule functions of limo-velo_amd/csrc/lv_surf_merge.hpp (what the kernel of lv_surf_merge.hip
runs) compiled with g++ and held to tests/surf_merge_ref.py on the generated cases of tests/surf_merge_cases.py, equality
everywhere: the lattice position, the state, dS and dW of every destination voxel, the volume after the call and the four stats.
The two shortcuts are held to the voxels the reference finds: a voxel that is not OUTSIDE is never outside surf_merge_box nor in a
tile that surf_merge_tile_outside gives up, at the kernel's tile of 16 x 4 x 4 voxels.  surf_merge_rule's refusals one by one.
tests/emu/surf_merge_emu.cpp, once plain and once under AddressSanitizer + UndefinedBehaviorSanitizer (a stand-alone program)."""
import glob
import os
import subprocess

import numpy as np
import pytest

import surf_merge_cases as mc
import surf_merge_ref as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")
BUILD_DIR = os.path.join(EMU_DIR, "_build")
CSRC = os.path.join(ROOT, "limo-velo_amd", "csrc")
SOURCES = [os.path.join(EMU_DIR, "surf_merge_emu.cpp"), os.path.join(EMU_DIR, "hip", "hip_runtime.h"),
           os.path.join(ROOT, "include", "limovelo_hip.h"), *sorted(glob.glob(os.path.join(CSRC, "*.hpp")))]
BUILDS = {"plain": [], "asan": ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]}
CASES = mc.cases()
F = np.float32


@pytest.fixture(scope="module")
def emu_bins():
    os.makedirs(BUILD_DIR, exist_ok=True)
    bins = {b: os.path.join(BUILD_DIR, "surf_merge_emu_" + b) for b in BUILDS}
    stale = [b for b, exe in bins.items()
             if not os.path.exists(exe) or any(os.path.getmtime(s) > os.path.getmtime(exe) for s in SOURCES)]
    procs = [(b, subprocess.Popen(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-ffp-contract=off", "-I" + EMU_DIR, *BUILDS[b],
                                   "-o", bins[b], SOURCES[0]], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
             for b in stale]
    for b, p in procs:
        out, _ = p.communicate()
        assert p.returncode == 0, f"{b} build failed:\n{out}"
    return bins


def _run(exe, mode, text):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, mode], input=text, capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and "runtime error" not in r.stderr, r.stderr[-4000:]
    return r.stdout.strip().split("\n")


def _b32(a):
    return " ".join(str(int(x)) for x in np.asarray(a, F).reshape(-1).view(np.uint32))


def _b64(a):
    return " ".join(str(int(x)) for x in np.asarray(a, np.float64).reshape(-1).view(np.uint64))


def _ints(a):
    return " ".join(str(int(x)) for x in np.asarray(a).reshape(-1))


def call_text(c):
    d, s = c["dest"], c["sub"]
    nz, ny, nx = d["S"].shape
    sz, sy, sx = s["S"].shape
    return "\n".join([f"{_b32(d['origin'])} {_b32(d['resolution'])} {nx} {ny} {nz} {d['trunc_cells']} {d['max_weight']}",
                      f"{_b32(s['origin'])} {_b32(s['resolution'])} {sx} {sy} {sz} {s['trunc_cells']}",
                      f"{_b64(c['pose'][0])} {_b64(c['pose'][1])} {c['min_weight']} {c['interp']}",
                      _ints(s["S"]), _ints(s["W"]), _ints(d["S"]), _ints(d["W"])]) + "\n"


@pytest.mark.parametrize("build", list(BUILDS))
@pytest.mark.parametrize("name", list(CASES))
def test_rule_equals_the_reference(emu_bins, name, build):
    c = CASES[name]
    want = mr.merge(c["dest"], c["sub"], c["pose"], c["min_weight"], c["interp"])
    out = _run(emu_bins[build], "merge", call_text(c))
    assert out[0] == f"rc 0 kq {want['kq']}"
    box = [int(v) for v in out[1].split()[1:]]
    wb = mr.box(c["dest"], c["sub"], c["pose"])   # (the box the non-vacuity test counts against is the one the kernel is launched over)
    assert box == ([0] * 7 if wb is None else [1, *wb[0], *wb[1]])
    stats = np.array(out[2].split()[1:], np.uint64)
    rec = np.array([o.split() for o in out[3:]], np.int64).reshape(*c["dest"]["S"].shape, 9)
    judged, state, dS, dW = rec[..., 0].astype(bool), rec[..., 1], rec[..., 2], rec[..., 3]
    assert np.array_equal(state, want["state"]) and np.array_equal(dS, want["dS"]) and np.array_equal(dW, want["dW"])
    far = want["state"] == mr.OUTSIDE   # (e means nothing where |u| >= 2^24; no case has such a voxel, so it is compared everywhere)
    for b in range(3):
        assert np.array_equal(rec[..., 4 + b], want["e"][b])
    # the shortcuts: nothing that is not OUTSIDE was left out, and what was left out changes nothing
    assert not (~far & ~judged).any(), "a voxel that is not OUTSIDE lies outside the box or in a tile given up"
    inside = np.zeros(far.shape, bool)
    if box[0]:
        assert all(0 <= box[1 + a] < box[4 + a] <= n for a, n in enumerate(far.shape[::-1]))
        inside[box[3]:box[6], box[2]:box[5], box[1]:box[4]] = True
    assert not (judged & ~inside).any() and not (~far & ~inside).any()
    assert np.array_equal(rec[..., 7], want["S"]) and np.array_equal(rec[..., 8], want["W"]) and np.array_equal(stats, want["stats"])
    if name == "misses":
        assert not box[0]
    if name == "grazes":
        assert box[0] and inside.sum() < inside.size // 4 and (inside & ~judged).any()   # both shortcuts cut


def test_shortcuts_do_cut(emu_bins):
    """Over the cases the box is smaller than the volume and tiles inside it are given up."""
    shrunk = culled = 0
    for c in CASES.values():
        out = _run(emu_bins["plain"], "merge", call_text(c))
        box = [int(v) for v in out[1].split()[1:]]
        rec = np.array([o.split() for o in out[3:]], np.int64).reshape(*c["dest"]["S"].shape, 9)
        inside = np.zeros(c["dest"]["S"].shape, bool)
        if box[0]:
            inside[box[3]:box[6], box[2]:box[5], box[1]:box[4]] = True
        shrunk += int(inside.sum() < inside.size)
        culled += int((inside & ~rec[..., 0].astype(bool)).any())
    assert shrunk >= 4 and culled >= 2


KQ_RANGE = "lv_surf_merge: the submap's resolution %s against the volume's %s: a ratio of 1/8 to 8"
RULES = [("ok 0", "ok 4096 1 0"), ("params 0", "ok 4096 1 0"), ("min_weight 7", "ok 4096 7 0"), ("interp 1", "ok 4096 1 1"), ("dest_resolution 0.16", "ok 5120 1 0"),
         ("dest_resolution 1.6", "ok 512 1 0"), ("dest_resolution 0.025", "ok 32768 1 0"), ("w5 262144", "ok 4096 1 0"), ("w5 0", "ok 4096 1 0"), ("s7 768", "ok 4096 1 0"),
         ("s7 -768", "ok 4096 1 0"), ("trunc_cells 16", "ok 4096 1 0"), ("qnorm 1.0000005", "ok 4096 1 0"),
         ("sub 0", "lv_surf_merge: null argument"), ("pose 0", "lv_surf_merge: null argument"),
         ("origin nan", "lv_surf_merge: submap origin: must be finite"), ("origin inf", "lv_surf_merge: submap origin: must be finite"),
         ("resolution 0", "lv_surf_merge: submap resolution = 0: finite and > 0"), ("resolution -0.2", "lv_surf_merge: submap resolution = -0.2: finite and > 0"),
         ("resolution inf", "lv_surf_merge: submap resolution = inf: finite and > 0"), ("resolution nan", "lv_surf_merge: submap resolution = nan: finite and > 0"),
         ("nx 0", "lv_surf_merge: submap of 0 x 3 x 2 voxels: each must be in 1..1024"), ("ny 1025", "lv_surf_merge: submap of 4 x 1025 x 2 voxels: each must be in 1..1024"),
         ("nz -1", "lv_surf_merge: submap of 4 x 3 x -1 voxels: each must be in 1..1024"),
         ("voxels 257", "lv_surf_merge: submap of 1024 x 1024 x 257 voxels: at most 2^28"),
         ("trunc_cells 0", "lv_surf_merge: submap trunc_cells = 0: must be in 1..16"), ("trunc_cells 17", "lv_surf_merge: submap trunc_cells = 17: must be in 1..16"),
         ("S 0", "lv_surf_merge: null S or W"), ("W 0", "lv_surf_merge: null S or W"),
         ("t nan", "lv_surf_merge: pose: t: a non-finite number"), ("t inf", "lv_surf_merge: pose: t: a non-finite number"),
         ("q nan", "lv_surf_merge: pose: q: a non-finite number"), ("q 0.01", "lv_surf_merge: pose: q: norm off 1 by more than 1e-6"),
         ("qnorm 1.00001", "lv_surf_merge: pose: q: norm off 1 by more than 1e-6"),
         ("min_weight 0", "lv_surf_merge: min_weight = 0: at least 1"), ("min_weight -3", "lv_surf_merge: min_weight = -3: at least 1"),
         ("interp 2", "lv_surf_merge: interp = 2: LV_MERGE_TRILINEAR or LV_MERGE_NEAREST"), ("interp -1", "lv_surf_merge: interp = -1: LV_MERGE_TRILINEAR or LV_MERGE_NEAREST"),
         ("w5 -1", "lv_surf_merge: submap voxel 5: S = 0, W = -1: 0 <= W <= 2^18 and |S| <= T * W"),
         ("w5 262145", "lv_surf_merge: submap voxel 5: S = 0, W = 262145: 0 <= W <= 2^18 and |S| <= T * W"),
         ("s7 769", "lv_surf_merge: submap voxel 7: S = 769, W = 1: 0 <= W <= 2^18 and |S| <= T * W"),
         ("s7 -769", "lv_surf_merge: submap voxel 7: S = -769, W = 1: 0 <= W <= 2^18 and |S| <= T * W"),
         ("dest_resolution 1.7", KQ_RANGE % ("0.2", "1.7")), ("dest_resolution 0.0249", KQ_RANGE % ("0.2", "0.0249"))]


@pytest.mark.parametrize("build", list(BUILDS))
def test_argument_rule(emu_bins, build):
    out = _run(emu_bins[build], "rule", "\n".join(r for r, _ in RULES) + "\n")
    assert out == [w for _, w in RULES]
