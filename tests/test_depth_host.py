"""Host tests of the depth fusion: the rule functions of limo-velo_amd/csrc/lv_depth.hpp (what the kernel of lv_depth.hip runs)
compiled with g++ and held to tests/depth_ref.py on generated records, equality everywhere; the two shortcuts against the voxels
the reference projects (a voxel that a view judges is never outside that view's box, nor inside a tile called unseen); depth_rule's
refusals one by one; and lv_depth_integrate's method of VolumeTools (lv_volumes.hpp) against stand-ins of the store's members.
tests/emu/depth_emu.cpp, once plain and once under AddressSanitizer + UndefinedBehaviorSanitizer (a stand-alone program)."""
import glob
import os
import subprocess

import numpy as np
import pytest

import depth_cases as dc
import depth_ref as dr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")
BUILD_DIR = os.path.join(EMU_DIR, "_build")
CSRC = os.path.join(ROOT, "limo-velo_amd", "csrc")
SOURCES = [os.path.join(EMU_DIR, "depth_emu.cpp"), os.path.join(EMU_DIR, "hip", "hip_runtime.h"),
           os.path.join(ROOT, "include", "limovelo_hip.h"), *sorted(glob.glob(os.path.join(CSRC, "*.hpp")))]
BUILDS = {"plain": [], "asan": ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]}
SCENARIOS = ["unconfigured", "integrate", "colour_untouched", "defaults"]
F = np.float32


@pytest.fixture(scope="module")
def emu_bins():
    os.makedirs(BUILD_DIR, exist_ok=True)
    bins = {b: os.path.join(BUILD_DIR, "depth_emu_" + b) for b in BUILDS}
    stale = [b for b, exe in bins.items()
             if not os.path.exists(exe) or any(os.path.getmtime(s) > os.path.getmtime(exe) for s in SOURCES)]
    procs = [(b, subprocess.Popen(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-ffp-contract=off", "-I" + EMU_DIR, *BUILDS[b],
                                   "-o", bins[b], SOURCES[0]], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
             for b in stale]
    for b, p in procs:
        out, _ = p.communicate()
        assert p.returncode == 0, f"{b} build failed:\n{out}"
    return bins


@pytest.mark.parametrize("build", list(BUILDS))
@pytest.mark.parametrize("scenario", SCENARIOS)
def test_depth_tools_scenario(emu_bins, scenario, build):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([emu_bins[build], scenario], capture_output=True, text=True, timeout=60, env=env)
    assert r.returncode == 0, f"{scenario} ({build}) exited {r.returncode}:\n{r.stderr[-4000:]}"
    assert "runtime error" not in r.stderr, r.stderr[-4000:]
    assert r.stdout.strip() == "ok " + scenario


def _run(emu_bins, lines):
    r = subprocess.run([emu_bins["asan"], "rule"], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "runtime error" not in r.stderr, r.stderr[-4000:]
    out = r.stdout.strip().split("\n")
    assert len(out) == len(lines)
    return out


def _bits(v):
    return int(np.asarray(v, F).reshape(1).view(np.uint32)[0])


def _b(a):
    return " ".join(str(_bits(x)) for x in np.asarray(a, F).reshape(-1))


def test_measured_depth(emu_bins):
    rng = np.random.default_rng(21)
    prm = dc.params(min_depth=0.3, max_depth=5.0)
    mn, mx = F(prm.min_depth), F(prm.max_depth)
    # U16: raw 0 and 65535, the raws round both limits at two scales, random ones
    for scale in (F(0.001), F(0.00025), F(0.005)):
        edge = [int(round(float(lim) / float(scale))) + d for lim in (mn, mx) for d in (-2, -1, 0, 1, 2)]
        raw = np.array([0, 1, 65535] + [e for e in edge if 0 <= e <= 65535] + list(rng.integers(0, 65536, 300)), np.uint16)
        out = np.array([o.split() for o in _run(emu_bins, [f"u16 {r} {_bits(scale)} {_bits(mn)} {_bits(mx)}" for r in raw])], np.int64)
        valid, D = dr.measured(raw, scale, prm)
        assert np.array_equal(out[:, 0], valid.astype(np.int64)) and not valid[0] and valid.any() and not valid.all()
        assert np.array_equal(out[raw != 0, 1], D[raw != 0].view(np.uint32))
    # F32: NaN, +-inf, -1, 0, the limits themselves and their neighbours
    vals = np.array([np.nan, np.inf, -np.inf, -1.0, 0.0, -0.0, mn, mx, np.nextafter(mn, F(0)), np.nextafter(mn, F(9)), np.nextafter(mx, F(0)),
                     np.nextafter(mx, F(9)), 1e-40, 3.4e38] + list(rng.uniform(-1, 7, 300)), F)
    out = np.array([o.split() for o in _run(emu_bins, [f"f32 {_bits(v)} {_bits(mn)} {_bits(mx)}" for v in vals])], np.int64)
    valid, D = dr.measured(vals, None, prm)
    assert np.array_equal(out[:, 0], valid.astype(np.int64)) and np.array_equal(out[:, 1], D.view(np.uint32))
    assert list(valid[:14]) == [False, False, False, False, False, False, True, True, False, True, True, False, False, False]


def test_quantised_distance(emu_bins):
    rng = np.random.default_rng(22)
    rows = []
    # q exactly -T - 1, -T, T, T + 1 (and the values between): resolution a power of two, D - z = res * (q + 0.5) / 256 exactly
    for tc in (1, 3, 16):
        T = 256 * tc
        for q in (-T - 2, -T - 1, -T, -T + 1, -1, 0, 1, T - 1, T, T + 1, T + 2):
            for res in (F(0.25), F(0.125)):
                z = F(1.0)
                D = F(z + res * F(q + 0.5) / F(256))
                rows.append((D, z, res, T))
                assert np.floor(((D - z) / res) * F(256)) == q
    # random pairs round the band at awkward resolutions
    for _ in range(3000):
        res = F(rng.choice([0.05, 0.1, 0.2, 0.37]))
        tc = int(rng.integers(1, 17))
        z = F(rng.uniform(0.3, 8.0))
        D = F(z + rng.uniform(-1.3, 1.3) * tc * res)
        rows.append((D, z, res, 256 * tc))
    for carve in (0, 1):
        out = np.array([o.split() for o in _run(emu_bins, [f"quant {_bits(D)} {_bits(z)} {_bits(r)} {T} {carve}" for D, z, r, T in rows])], np.int64)
        seen = set()
        for (D, z, r, T), (adds, s) in zip(rows, out):
            a, want, q = dr.quantise(np.array([D], F), np.array([z], F), r, T, carve)
            assert (int(adds), int(s)) == (int(a[0]), int(want[0]) if a[0] else 0), (D, z, r, T, carve)
            seen.add("behind" if q[0] < -T else "far" if q[0] > T else "band")
        assert seen == {"behind", "far", "band"}


def test_shortcuts_never_drop_a_projected_voxel(emu_bins):
    """depth_view_box and depth_box_unseen against the reference's projection of every voxel: the scene's views, a distorted one,
    the corner camera, the 1 x 1 image and 32 more, at the kernel's tile of 64 x 4 x 1 voxels."""
    shape = (dc.NZ, dc.NY, dc.NX)
    cases = [(f, dc.params()) for f in dc.frames3() + [dc.frame_distorted(), dc.frame_pixel()] + dc.frames32()[:6]]
    cases += [(dc.frame_corner(), dc.params(max_depth=1.2)), (dc.frame_nothing(), dc.params()), (dc.frame(), dc.params(max_norm_radius=0.4, max_depth=1.5))]
    X, Y, Z = dr.centres(dc.ORIGIN, dc.RES, shape)
    grid = f"{_b(dc.ORIGIN)} {_bits(dc.RES)} {dc.NX} {dc.NY} {dc.NZ}"
    lines, tiles = [], []
    for f, p in cases:
        lines.append(f"viewbox {grid} {_b(f['R'])} {_b(f['t'])} {_bits(p.max_depth)} {_bits(p.max_norm_radius)}")
    for f, p in cases:
        for k in range(dc.NZ):
            for j0 in range(0, dc.NY, 4):
                j1 = min(j0 + 4, dc.NY) - 1
                lo = (X[k, j0, 0], Y[k, j0, 0], Z[k, j0, 0])
                hi = (X[k, j1, dc.NX - 1], Y[k, j1, dc.NX - 1], Z[k, j1, dc.NX - 1])
                tiles.append((len(lines), k, j0, j1))
                lines.append(f"unseen {_b(f['R'])} {_b(f['t'])} {_bits(p.min_depth)} {_bits(p.max_depth)} {_bits(p.max_norm_radius)} {_b(lo)} {_b(hi)}")
    out = _run(emu_bins, lines)
    oks = [dr.project(X, Y, Z, f, p)[0] for f, p in cases]
    shrunk = culled = 0
    for c, ok in enumerate(oks):
        any_, x0, y0, z0, x1, y1, z1 = (int(v) for v in out[c].split())
        inside = np.zeros(shape, bool)
        if any_:
            assert 0 <= x0 < x1 <= dc.NX and 0 <= y0 < y1 <= dc.NY and 0 <= z0 < z1 <= dc.NZ
            inside[z0:z1, y0:y1, x0:x1] = True
        assert not (ok & ~inside).any(), f"case {c}: a projected voxel lies outside the view's box"
        shrunk += int(inside.sum() < inside.size)
    per = len(tiles) // len(cases)
    for n, (line, k, j0, j1) in enumerate(tiles):
        if int(out[line]):
            culled += 1
            assert not oks[n // per][k, j0:j1 + 1, :].any(), f"case {n // per}: tile ({k}, {j0}) is called unseen and holds a projected voxel"
    assert not int(out[len(cases) - 2].split()[0]) and shrunk >= 3 and culled > 100   # the shortcuts do cut: the far camera sees nothing at all


RULES = [("ok 0", "ok 1 256"), ("n_views 32", "ok 32 8192"), ("total 4", "ok 4 134217728"), ("carve 1", "ok 1 256"),
         ("f32_stride 12", "ok 1 256"), ("f32_scale 0", "ok 1 256"), ("f32_scale nan", "ok 1 256"),   # depth_scale is ignored for F32
         ("views 0", "lv_depth_integrate: null argument"), ("params 0", "lv_depth_integrate: null argument"),
         ("n_views 0", "lv_depth_integrate: n_views = 0: must be in 1..32"), ("n_views 33", "lv_depth_integrate: n_views = 33: must be in 1..32"),
         ("min_depth 0", "lv_depth_integrate: depths [0, 10]: finite, 0 < min_depth < max_depth"),
         ("min_depth 10", "lv_depth_integrate: depths [10, 10]: finite, 0 < min_depth < max_depth"),
         ("max_depth inf", "lv_depth_integrate: depths [0.3, inf]: finite, 0 < min_depth < max_depth"),
         ("min_depth nan", "lv_depth_integrate: depths [nan, 10]: finite, 0 < min_depth < max_depth"),
         ("max_norm_radius 0", "lv_depth_integrate: max_norm_radius = 0: finite and > 0"),
         ("max_norm_radius inf", "lv_depth_integrate: max_norm_radius = inf: finite and > 0"),
         ("carve 2", "lv_depth_integrate: carve = 2: 0 or 1"), ("carve -1", "lv_depth_integrate: carve = -1: 0 or 1"),
         ("R inf", "lv_depth_integrate: view 0: non-finite R"), ("t nan", "lv_depth_integrate: view 0: non-finite t"),
         ("fx inf", "lv_depth_integrate: view 0: non-finite intrinsics"), ("cy nan", "lv_depth_integrate: view 0: non-finite intrinsics"),
         ("dist nan", "lv_depth_integrate: view 0: non-finite distortion"),
         ("width 0", "lv_depth_integrate: view 0: image of 0 x 2 pixels: each side 1..8192, at most 2^24 in all"),
         ("height 8193", "lv_depth_integrate: view 0: image of 3 x 8193 pixels: each side 1..8192, at most 2^24 in all"),
         ("side 8192", "lv_depth_integrate: view 0: image of 8192 x 8192 pixels: each side 1..8192, at most 2^24 in all"),
         ("format 2", "lv_depth_integrate: view 0: format 2"), ("format -1", "lv_depth_integrate: view 0: format -1"),
         ("depth_scale 0", "lv_depth_integrate: view 0: depth_scale = 0: finite and > 0"),
         ("depth_scale -0.001", "lv_depth_integrate: view 0: depth_scale = -0.001: finite and > 0"),
         ("depth_scale inf", "lv_depth_integrate: view 0: depth_scale = inf: finite and > 0"),
         ("depth 0", "lv_depth_integrate: view 0: null depth or row_stride 6 < 6"),
         ("row_stride 5", "lv_depth_integrate: view 0: null depth or row_stride 5 < 6"),
         ("f32_stride 11", "lv_depth_integrate: view 0: null depth or row_stride 11 < 12"),
         ("total 5", "lv_depth_integrate: the views hold more than 2^26 pixels together")]


def test_argument_rule(emu_bins):
    out = _run(emu_bins, ["rule " + r for r, _ in RULES])
    assert out == [w for _, w in RULES]
