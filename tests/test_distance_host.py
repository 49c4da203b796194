"""The rule of lv_distance.hpp (the obstacle test, the X / Y / Z passes, truncation, metres, query and gradient: what the kernels of
lv_distance.hip run) compiled with g++ and -fsanitize=address,undefined through tests/emu/hip/hip_runtime.h and held to
tests/distance_ref.py: tests/emu/distance_emu.cpp builds the field of the given log-odds and prints s2, the metres' bits, the stats
and the answers to the query points.  Equality on every voxel, no tolerance."""
import os
import subprocess

import numpy as np
import pytest

import distance_ref as dr
import occupancy_ref as ocr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")
CSRC = os.path.join(ROOT, "limo-velo_amd", "csrc")
F = np.float32


def _bits(values):
    return " ".join(str(int(v)) for v in np.asarray(values, F).reshape(-1).view(np.uint32))


def emu_input(prm, dp, L, pts):
    pts = np.asarray(pts, F).reshape(-1, 3)
    lines = [" ".join([_bits(prm["origin"]), _bits([prm["resolution"]]), str(prm["nx"]), str(prm["ny"]), str(prm["nz"]),
                       _bits([prm["l_occ"], prm["l_free"]])]),
             " ".join(str(int(dp[f])) for f in dr.FIELDS), _bits(L), str(len(pts)), _bits(pts)]
    return ("\n".join(lines) + "\n").encode()


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    exe = tmp_path_factory.mktemp("distance_host") / "distance_emu"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I" + EMU_DIR, "-I" + CSRC, os.path.join(EMU_DIR, "distance_emu.cpp"), "-o",
                           str(exe)])

    def run(prm, dp, L, pts=()):
        out = subprocess.run([str(exe)], input=emu_input(prm, dp, L, pts), stdout=subprocess.PIPE, check=True).stdout.decode().split("\n")
        if out[0] != "params ok":
            return out[0]
        head = out[1].split()
        assert head[0] == "field"
        nx, ny, nz = (int(v) for v in head[1:])
        shape = (ny, nx) if dp["planar"] else (nz, ny, nx)
        s2 = np.array(out[2].split(), np.int64).astype(np.int32).reshape(shape)
        met = np.array(out[3].split(), np.uint32).view(F).reshape(shape)
        st = out[4].split()
        assert st[0] == "stats"
        q = np.array([ln.split() for ln in out[5:5 + len(pts)]], np.uint32).view(F).reshape(-1, 4)
        return s2, met, np.array(st[1:], np.uint64), q[:, 0], q[:, 1:]

    return run


def _hold(emu, prm, dp, L, pts):
    s2, met, st, dist, grad = emu(prm, dp, L, pts)
    rs2, rst = dr.build(prm, L, dp)
    assert np.array_equal(s2, rs2), f"{np.sum(s2 != rs2)} values differ"
    assert dr.same_bits(met, dr.metres(rs2, prm["resolution"]))
    assert list(st) == list(rst)
    rd, rg = dr.query(prm, dp, rs2, pts)
    assert dr.same_bits(dist, rd) and dr.same_bits(grad, rg)
    return s2


PARAMS = [dr.dparams(), dr.dparams(signed_field=1), dr.dparams(unknown_is_obstacle=1, signed_field=1), dr.dparams(max_cells=1),
          dr.dparams(max_cells=3, signed_field=1), dr.dparams(planar=1, k_lo=-2, k_hi=99, signed_field=1),
          dr.dparams(planar=1, k_lo=1, k_hi=2, unknown_is_obstacle=1, max_cells=3)]


@pytest.mark.parametrize("dims", [(12, 9, 7), (33, 5, 3), (31, 2, 4), (1, 6, 5), (65, 1, 2), (1, 1, 1)])
def test_random_grids(emu, dims):
    nx, ny, nz = dims
    rng = np.random.default_rng(nx + 7 * ny)
    prm = ocr.params(origin=(-1.0, 0.5, 2.0), resolution=0.25, nx=nx, ny=ny, nz=nz)
    pts = dr.probe_points(prm, rng, 40, 60)
    n = nx * ny * nz
    one = np.full(n, -1.0, F)
    one[rng.integers(n)] = 2.0
    grids = [np.full((nz, ny, nx), np.nan, F), one.reshape(nz, ny, nx), dr.random_logodds(rng, (nz, ny, nx), 0.05, prm=prm),
             dr.random_logodds(rng, (nz, ny, nx), 0.5, 0.2, prm=prm), np.full((nz, ny, nx), 3.5, F)]
    for L in grids:
        for dp in PARAMS:
            _hold(emu, prm, dp, L, pts)


def test_the_longest_axis(emu):
    rng = np.random.default_rng(5)
    prm = ocr.params(origin=(0.0, 0.0, 0.0), resolution=0.1, nx=1024, ny=2, nz=2)
    L = np.full((2, 2, 1024), -1.0, F)
    L[1, 1, 1023] = 1.0   # one obstacle in a corner: the longest diagonal
    pts = dr.probe_points(prm, rng, 20, 40)
    s2 = _hold(emu, prm, dr.dparams(), L, pts)
    assert s2[0, 0, 0] == 1023 ** 2 + 2 and s2.max() == 1023 ** 2 + 2
    _hold(emu, prm, dr.dparams(signed_field=1, max_cells=1024), L, pts)
    s2 = _hold(emu, prm, dr.dparams(max_cells=1000), L, pts)
    assert s2[0, 0, 0] == dr.FAR and s2[1, 1, 23] == 1000 ** 2 and s2[1, 0, 23] == dr.FAR
    _hold(emu, prm, dr.dparams(signed_field=1), dr.random_logodds(rng, (2, 2, 1024), 0.01, prm=prm), pts)
    _hold(emu, prm, dr.dparams(signed_field=1, unknown_is_obstacle=1), dr.random_logodds(rng, (2, 2, 1024), 0.6, prm=prm), pts)


def test_limits_are_refused(emu):
    prm = ocr.params(nx=3, ny=2, nz=2)
    L = np.zeros((2, 2, 3), F)
    for kw in (dict(max_cells=-1), dict(max_cells=1025), dict(planar=1, k_lo=3, k_hi=2)):
        out = emu(prm, dr.dparams(**kw), L)
        assert isinstance(out, str) and out.startswith("params bad"), kw
    for kw in (dict(max_cells=1024), dict(k_lo=3, k_hi=2), dict(planar=1, k_lo=2, k_hi=2), dict(planar=1, k_lo=-9, k_hi=-8)):
        assert not isinstance(emu(prm, dr.dparams(**kw), L), str), kw
