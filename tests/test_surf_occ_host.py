"""Host tests of lv_occ_from_surface's rule: the functions of limo-velo_amd/csrc/lv_surf_occ.hpp (what the kernels of lv_surf_occ.hip
run) compiled with g++ and run voxel by voxel over the scene of tests/surf_occ_cases.py, held to tests/surf_occ_ref.py by equality
on every bit of the grid and on all four stats, in all four modes, from a grid of random NaN / values in [l_min, l_max]; the
parameter check's refusals one by one; the defaults.  tests/emu/surf_occ_emu.cpp, once plain and once under AddressSanitizer +
UndefinedBehaviorSanitizer (a stand-alone program).  The same run holds surf_occ_axis_range, by which the device limits its bitmap
passes, to the TSDF voxels the box's voxels do fall into."""
import glob
import os
import struct
import subprocess

import numpy as np
import pytest

import surf_occ_cases as sc
import surf_occ_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")
BUILD_DIR = os.path.join(EMU_DIR, "_build")
CSRC = os.path.join(ROOT, "limo-velo_amd", "csrc")
SOURCES = [os.path.join(EMU_DIR, "surf_occ_emu.cpp"), os.path.join(EMU_DIR, "hip", "hip_runtime.h"),
           os.path.join(ROOT, "include", "limovelo_hip.h"), *sorted(glob.glob(os.path.join(CSRC, "*.hpp")))]
BUILDS = {"plain": [], "asan": ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]}
F = np.float32
MODES = {"fill": sr.FILL, "overwrite": sr.OVERWRITE, "replace": sr.REPLACE, "accumulate": sr.ACCUMULATE}


@pytest.fixture(scope="module")
def emu_bins():
    os.makedirs(BUILD_DIR, exist_ok=True)
    bins = {b: os.path.join(BUILD_DIR, "surf_occ_emu_" + b) for b in BUILDS}
    stale = [b for b, exe in bins.items()
             if not os.path.exists(exe) or any(os.path.getmtime(s) > os.path.getmtime(exe) for s in SOURCES)]
    procs = [(b, subprocess.Popen(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-ffp-contract=off", "-I" + EMU_DIR, *BUILDS[b],
                                   "-o", bins[b], SOURCES[0]], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
             for b in stale]
    for b, p in procs:
        out, _ = p.communicate()
        assert p.returncode == 0, f"{b} build failed:\n{out}"
    return bins


@pytest.fixture(scope="module")
def vol():
    return sc.volume()


def _geom(g):
    nz, ny, nx = g["shape"]
    return struct.pack("3f", *[float(v) for v in g["origin"]]), float(g["resolution"]), (nx, ny, nz)


def _emu(exe, tmp_path, grid, v, S, W, L, **kw):
    """one run of the emulator; (L', stats)"""
    p = dict(lo=(0, 0, 0), hi=(1 << 30,) * 3, min_weight=1, band=0, reach=0, mode=sr.FILL, l_solid=3.5, l_open=-2.0)
    p.update(kw)
    go, gr, gn = _geom(grid)
    vo, vr, vn = _geom(v)
    blob = go + struct.pack("3f3i", gr, sc.L_MIN, sc.L_MAX, *gn) + vo + struct.pack("f3i", vr, *vn)
    blob += struct.pack("6i4i2f", *p["lo"], *p["hi"], p["min_weight"], p["band"], p["reach"], p["mode"], p["l_solid"], p["l_open"])
    blob += np.ascontiguousarray(S, np.int32).tobytes() + np.ascontiguousarray(W, np.int32).tobytes() + np.ascontiguousarray(L, F).tobytes()
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    src.write_bytes(blob)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, "run", str(src), str(dst)], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and "runtime error" not in r.stderr, r.stderr[-4000:]
    raw = dst.read_bytes()
    return np.frombuffer(raw, F, offset=32).reshape(grid["shape"]), np.frombuffer(raw, np.uint64, 4)


def _hold(exe, tmp_path, grid, v, S, W, L, what, **kw):
    got, st = _emu(exe, tmp_path, grid, v, S, W, L, **kw)
    want, wst = sr.from_surface(L, grid, v, S, W, sc.L_MIN, sc.L_MAX, **kw)
    diff = int((got.view(np.uint32) != want.view(np.uint32)).sum())
    print(f"{what}: stats {st} (reference {wst}), {diff} voxels differ")
    assert np.array_equal(st, wst) and diff == 0, what
    return got, st


@pytest.mark.parametrize("name,min_weight,band,reach", sc.combinations())
def test_the_27_combinations(emu_bins, tmp_path, vol, name, min_weight, band, reach):
    grid = sc.grid_geometry(name)
    L = sc.random_grid(grid["shape"], 11)
    _, st = _hold(emu_bins["asan"], tmp_path, grid, sc.vol_geometry(), *vol, L, f"{name} {min_weight} {band} {reach}", min_weight=min_weight, band=band,
                  reach=reach, mode=sr.REPLACE)
    assert st[0] >= 84 and st[1] >= 84 and st[2] > 0


@pytest.mark.parametrize("build", list(BUILDS))
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", list(sc.GRIDS))
def test_the_four_modes(emu_bins, tmp_path, vol, name, mode, build):
    grid = sc.grid_geometry(name)
    nz, ny, nx = grid["shape"]
    L = sc.random_grid(grid["shape"], 12)
    for lo, hi in (((0, 0, 0), (1 << 30,) * 3), ((3, 2, 1), (nx - 4, ny - 3, nz - 2)), ((-5, -1, -2), (nx + 3, ny, nz + 7))):
        got, st = _hold(emu_bins[build], tmp_path, grid, sc.vol_geometry(), *vol, L, f"{name} {mode} box {lo}..{hi}", lo=lo, hi=hi, reach=1, band=64,
                        mode=MODES[mode], l_solid=0.9, l_open=-0.7)
        assert st[2] > 0
    # the clamps: l_solid and l_open beyond the grid's own
    _hold(emu_bins[build], tmp_path, grid, sc.vol_geometry(), *vol, L, f"{name} {mode} clamped", mode=MODES[mode], l_solid=9.0, l_open=-9.0)


def test_shifted_volumes_and_degenerate_cases(emu_bins, tmp_path, vol):
    S, W = vol
    exe = emu_bins["asan"]
    grid, v = sc.grid_geometry("coarse", (-5, 4, 0)), sc.vol_geometry((3, -2, 1))
    L = sc.random_grid(grid["shape"], 13)
    _, st = _hold(exe, tmp_path, grid, v, S, W, L, "both shifted", mode=sr.REPLACE, reach=3)
    assert st[0] > 0 and st[3] > 0
    # a grid far from the volume: everything OUTSIDE; an axis that does not quantise (65536 voxels and more away)
    for origin in ((100.0, 0.0, 0.0), (0.0, -3.0e4, 0.0), (0.0, 0.0, 1.0e30)):
        far = sr.geometry(origin, 0.4, (3, 4, 5))
        Lf = sc.random_grid((3, 4, 5), 14)
        got, st = _hold(exe, tmp_path, far, sc.vol_geometry(), S, W, Lf, f"far {origin}", mode=sr.REPLACE, reach=4)
        assert list(st) == [0, 0, int((Lf.view(np.uint32) != sr.NAN_BITS).sum()), 60] and st[2] > 20   # (every observed voxel becomes unknown)
        assert (got.view(np.uint32) == sr.NAN_BITS).all()
    # an empty box, a never observed volume, min_weight above every W, the band's ends
    grid = sc.grid_geometry("same")
    L = sc.random_grid(grid["shape"], 15)
    got, st = _hold(exe, tmp_path, grid, sc.vol_geometry(), S, W, L, "empty box", lo=(5, 5, 5), hi=(4, 9, 9), mode=sr.REPLACE)
    assert not st.any() and np.array_equal(got.view(np.uint32), L.view(np.uint32))
    _, st = _hold(exe, tmp_path, grid, sc.vol_geometry(), 0 * S, 0 * W, L, "never observed", mode=sr.ACCUMULATE, reach=4)
    assert not st.any()
    _, st = _hold(exe, tmp_path, grid, sc.vol_geometry(), S, W, L, "min_weight 6", mode=sr.OVERWRITE, min_weight=6)
    assert not st.any()
    _, st = _hold(exe, tmp_path, grid, sc.vol_geometry(), S, W, L, "band 4096", mode=sr.REPLACE, band=4096)
    assert st[0] == (W > 0).sum() and st[1] == 0
    _, st = _hold(exe, tmp_path, grid, sc.vol_geometry(), S, W, L, "band -4096", mode=sr.REPLACE, band=-4096)
    assert st[0] == 0 and st[1] == (W > 0).sum()


def _bits(v):
    return int(np.asarray(v, F).reshape(1).view(np.uint32)[0])


CHECKS = [((1, 0, 0, 0, 3.5, -2.0), "ok"), ((1 << 18, 4096, 4, 3, 1e-30, -1e-30), "ok"), ((1, -4096, 0, 2, 3e38, -3e38), "ok"),
          (None, "null params"),
          ((0, 0, 0, 0, 3.5, -2.0), "min_weight = 0: must be in 1..2^18"), (((1 << 18) + 1, 0, 0, 0, 3.5, -2.0), "min_weight = 262145: must be in 1..2^18"),
          ((1, 4097, 0, 0, 3.5, -2.0), "band = 4097: must be in -4096..4096"), ((1, -4097, 0, 0, 3.5, -2.0), "band = -4097: must be in -4096..4096"),
          ((1, 0, -1, 0, 3.5, -2.0), "reach = -1: must be in 0..4"), ((1, 0, 5, 0, 3.5, -2.0), "reach = 5: must be in 0..4"),
          ((1, 0, 0, -1, 3.5, -2.0), "mode = -1: must be in 0..3"), ((1, 0, 0, 4, 3.5, -2.0), "mode = 4: must be in 0..3"),
          ((1, 0, 0, 0, 0.0, -2.0), "l_solid = 0: finite and > 0"), ((1, 0, 0, 0, float("nan"), -2.0), "l_solid = nan: finite and > 0"),
          ((1, 0, 0, 0, float("inf"), -2.0), "l_solid = inf: finite and > 0"), ((1, 0, 0, 0, -1.0, -2.0), "l_solid = -1: finite and > 0"),
          ((1, 0, 0, 0, 3.5, 0.0), "l_open = 0: finite and < 0"), ((1, 0, 0, 0, 3.5, float("nan")), "l_open = nan: finite and < 0"),
          ((1, 0, 0, 0, 3.5, float("-inf")), "l_open = -inf: finite and < 0"), ((1, 0, 0, 0, 3.5, 2.0), "l_open = 2: finite and < 0"),
          ((0, 4097, 9, 9, 0.0, 0.0), "min_weight = 0: must be in 1..2^18")]   # (the first in the struct's order is reported)


def test_parameter_check_and_defaults(emu_bins):
    lines = ["null" if c is None else "%d %d %d %d %d %d" % (*c[:4], _bits(c[4]), _bits(c[5])) for c, _ in CHECKS]
    r = subprocess.run([emu_bins["asan"], "check"], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert r.stdout.strip().split("\n") == [w for _, w in CHECKS]
    r = subprocess.run([emu_bins["plain"], "defaults"], capture_output=True, text=True, timeout=60)
    assert r.stdout.split() == [str(v) for v in (0, 0, 0, 1 << 30, 1 << 30, 1 << 30, 1, 0, 0, 0, _bits(3.5), _bits(-2.0))]
