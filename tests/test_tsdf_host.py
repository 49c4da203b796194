"""The rule of lv_tsdf.hpp (the ray, the signed distance of a cell, the packed scratch word, the fold, the mesh: what the kernels of
lv_tsdf.hip run) compiled with g++ and -fsanitize=address,undefined through tests/emu/hip/hip_runtime.h and held to
tests/tsdf_ref.py on the shared cases of tests/tsdf_cases.py: S, W, metres, the stats of every call, the vertices and the
triangles.  Equality everywhere, no tolerance."""
import os
import subprocess

import numpy as np
import pytest

import tsdf_cases as tc
import tsdf_ref as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")
CSRC = os.path.join(ROOT, "limo-velo_amd", "csrc")
F = np.float32


def _bits(values):
    return " ".join(str(int(v)) for v in np.asarray(values, F).reshape(-1).view(np.uint32))


def emu_input(prm, calls, min_weight):
    head = " ".join([_bits(prm["origin"]), _bits([prm["resolution"]]), str(prm["nx"]), str(prm["ny"]), str(prm["nz"]),
                     _bits([prm["min_range"], prm["max_range"]]), str(prm["trunc_cells"]), str(prm["max_weight"]), str(prm["carve"]),
                     str(min_weight)])
    lines = [head, str(len(calls))]
    for views in calls:
        lines.append(str(len(views)))
        for R, t, pts in views:
            pts = np.asarray(pts, F).reshape(-1, 3)
            lines.append(" ".join([_bits(R), _bits(t), str(len(pts)), _bits(pts)]))
    return ("\n".join(lines) + "\n").encode()


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    exe = tmp_path_factory.mktemp("tsdf_host") / "tsdf_emu"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I" + EMU_DIR, "-I" + CSRC, os.path.join(EMU_DIR, "tsdf_emu.cpp"), "-o", str(exe)])

    def run(prm, calls, min_weight=1):
        out = subprocess.run([str(exe)], input=emu_input(prm, calls, min_weight), stdout=subprocess.PIPE, check=True).stdout.decode().split("\n")
        if out[0] != "params ok":
            return out[0]
        shape = (prm["nz"], prm["ny"], prm["nx"])
        stats = []
        for c in range(len(calls)):
            head = out[1 + c].split()
            assert head[0] == "call"
            stats.append(np.array(head[1:], np.uint64))
        o = 1 + len(calls)
        assert (out[o], out[o + 2], out[o + 4]) == ("S", "W", "metres")
        S = np.array(out[o + 1].split(), np.int32).reshape(shape)
        W = np.array(out[o + 3].split(), np.int32).reshape(shape)
        m = np.array(out[o + 5].split(), np.uint32).view(F).reshape(shape)
        head = out[o + 6].split()
        assert head[0] == "mesh"
        mesh = dict(counts=np.array(head[1:], np.uint64), sub=np.array(out[o + 7].split(), np.int32).reshape(-1, 3),
                    xyz=np.array(out[o + 8].split(), np.uint32).view(F).reshape(-1, 3), tri=np.array(out[o + 9].split(), np.uint32).reshape(-1, 3))
        return dict(S=S, W=W, metres=m, stats=stats, mesh=mesh)

    return run


def _same_mesh(got, ref):
    assert np.array_equal(got["counts"], ref["counts"])
    assert np.array_equal(got["sub"], ref["sub"])
    assert np.array_equal(got["xyz"].view(np.uint32), ref["xyz"].view(np.uint32))
    assert np.array_equal(got["tri"], ref["tri"])


@pytest.mark.parametrize("case", tc.cases(), ids=lambda c: c["name"])
def test_shared_cases(emu, case):
    got = emu(case["prm"], case["calls"], case["min_weight"])
    ref = tc.reference(case)
    assert [list(s) for s in got["stats"]] == [list(s) for s in ref["stats"]]
    assert np.array_equal(got["S"], ref["S"]) and np.array_equal(got["W"], ref["W"])
    assert tr.same_metres(got["metres"], tr.metres(case["prm"], ref["S"], ref["W"]))
    _same_mesh(got["mesh"], ref["mesh"])


def test_degenerate_rays_and_tiny_grids(emu):
    """Axis-parallel and diagonal rays from a voxel's centre and from a lattice corner, a return in the sensor's own sub-unit
    (len = 0), grids with a dimension of 1 (no cell exists: an empty mesh)."""
    ax = [(sgn * r * np.eye(3)[a]) for a in range(3) for sgn in (1, -1) for r in (0.3, 0.5, 1.0, 3.0, 5.0)]
    diag = [np.array([sx, sy, sz]) * r for sx in (1, -1) for sy in (1, -1) for sz in (1, -1) for r in (0.25, 0.75, 1.0, 2.5)]
    pts = np.array(ax + diag, F)
    for carve in (0, 1):
        prm = tc.grid_params(19, 13, 9, carve=carve)
        for t in ((0.125, 0.125, 0.125), (0.0, 0.0, 0.0), (0.25, 0.1, 0.1)):
            calls = [[(tc.ID, np.array(t, F), pts)]]
            got = emu(prm, calls)
            S, W, st = tr.integrate(prm, *tr.empty(prm), calls[0])
            assert np.array_equal(got["S"], S) and np.array_equal(got["W"], W) and list(got["stats"][0]) == list(st)
            _same_mesh(got["mesh"], tr.mesh(prm, S, W))
    # len = 0: min_range below a sub-unit lets a return quantise onto the sensor
    prm = tr.params(origin=(0.0, 0.0, 0.0), resolution=1.0, nx=4, ny=4, nz=4, min_range=1e-4, max_range=3.0, trunc_cells=1)
    calls = [[(tc.ID, np.array([1.5, 1.5, 1.5], F), np.array([[1e-3, 0, 0], [1.0, 0, 0]], F))]]
    got = emu(prm, calls)
    S, W, st = tr.integrate(prm, *tr.empty(prm), calls[0])
    assert list(st) == [1, 0, 3, 3] and list(got["stats"][0]) == list(st)
    assert np.array_equal(got["S"], S) and np.array_equal(got["W"], W)
    for nx, ny, nz in ((1, 5, 4), (6, 1, 3), (5, 4, 1), (1, 1, 1)):
        prm = tr.params(origin=(0.0, 0.0, 0.0), resolution=0.5, nx=nx, ny=ny, nz=nz, min_range=0.05, max_range=10.0, trunc_cells=2)
        rng = np.random.default_rng(nx + 10 * ny)
        hi = np.array([nx, ny, nz]) * 0.5
        t = (hi + 0.7).astype(F)
        ends = rng.uniform(-1.0, 1.0, (200, 3)) * (hi + 2.0) + hi * 0.5
        calls = [[(tc.ID, t, (ends - t).astype(F))]]
        got = emu(prm, calls)
        S, W, st = tr.integrate(prm, *tr.empty(prm), calls[0])
        assert np.array_equal(got["S"], S) and np.array_equal(got["W"], W) and list(got["stats"][0]) == list(st)
        assert list(got["mesh"]["counts"][:3]) == [0, 0, 0]
        _same_mesh(got["mesh"], tr.mesh(prm, S, W))


def test_limits_are_refused(emu):
    prm = tc.grid_params(5, 4, 3)
    got = emu(prm, [])
    assert not got["W"].any() and list(got["mesh"]["counts"]) == [0, 0, 0, 0]
    bad = [dict(nx=0), dict(ny=1025), dict(nz=0), dict(nx=1024, ny=1024, nz=257), dict(resolution=0.0), dict(resolution=np.inf),
           dict(max_range=0.25 * 4096 * 1.01), dict(min_range=0.0), dict(min_range=7.0), dict(origin=(np.nan, 0.0, 0.0)), dict(trunc_cells=0),
           dict(trunc_cells=17), dict(max_weight=0), dict(max_weight=2 ** 18 + 1), dict(carve=2), dict(carve=-1)]
    for kw in bad:
        out = emu(dict(prm, **kw), [])
        assert isinstance(out, str) and out.startswith("params bad"), kw
    for kw in (dict(max_range=0.25 * 4096), dict(trunc_cells=16), dict(max_weight=2 ** 18), dict(trunc_cells=1, max_weight=1, carve=1)):
        assert not isinstance(emu(dict(prm, **kw), []), str), kw
