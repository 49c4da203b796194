"""The rule of lv_occupancy.hpp (quantisation, range rules, the integer walk, the update: what the kernels of lv_occupancy.hip run)
compiled with g++ and -fsanitize=address,undefined through tests/emu/hip/hip_runtime.h and held to tests/occupancy_ref.py:
tests/emu/occupancy_emu.cpp integrates the given views and prints each view's free and hit voxels, the stats and the grid's bits.
Equality on every voxel, no tolerance."""
import os
import subprocess

import numpy as np
import pytest

import occupancy_ref as ocr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")
CSRC = os.path.join(ROOT, "limo-velo_amd", "csrc")
F = np.float32


def _bits(values):
    return " ".join(str(int(v)) for v in np.asarray(values, F).reshape(-1).view(np.uint32))


def emu_input(prm, views):
    head = " ".join([_bits(prm["origin"]), _bits([prm["resolution"]]), str(prm["nx"]), str(prm["ny"]), str(prm["nz"]),
                     _bits([prm[k] for k in ("min_range", "max_range", "l_hit", "l_miss", "l_min", "l_max", "l_occ", "l_free")])])
    lines = [head, str(len(views))]
    for R, t, pts in views:
        pts = np.asarray(pts, F).reshape(-1, 3)
        lines.append(" ".join([_bits(R), _bits(t), str(len(pts)), _bits(pts)]))
    return ("\n".join(lines) + "\n").encode()


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    exe = tmp_path_factory.mktemp("occupancy_host") / "occupancy_emu"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I" + EMU_DIR, "-I" + CSRC, os.path.join(EMU_DIR, "occupancy_emu.cpp"), "-o",
                           str(exe)])

    def run(prm, views):
        out = subprocess.run([str(exe)], input=emu_input(prm, views), stdout=subprocess.PIPE, check=True).stdout.decode().split("\n")
        if out[0] != "params ok":
            return out[0]
        per_view = []
        for v in range(len(views)):
            head = out[1 + 3 * v].split()
            assert head[0] == "view"
            per_view.append((np.array(head[1:], np.uint64), np.array(out[2 + 3 * v].split(), np.int64), np.array(out[3 + 3 * v].split(), np.int64)))
        assert out[1 + 3 * len(views)] == "grid"
        L = np.array(out[2 + 3 * len(views)].split(), np.uint32).view(F).reshape(prm["nz"], prm["ny"], prm["nx"])
        return per_view, L

    return run


def _hold(emu, prm, views):
    """The emulation equals the reference: per view the sets and the stats, at the end the grid."""
    per_view, L = emu(prm, views)
    ref = ocr.empty(prm)
    for (stats, free, hit), (R, t, pts) in zip(per_view, views):
        rf, rh, used, cut = ocr.view_sets(prm, R, t, pts)
        assert np.array_equal(free, np.nonzero(rf.reshape(-1))[0])
        assert np.array_equal(hit, np.nonzero(rh.reshape(-1))[0])
        assert list(stats) == [used, cut, rf.sum(), rh.sum()]
        ref = ocr.update(prm, ref, rf, rh)
    assert ocr.same_bits(L, ref)
    return L, per_view


def _rot(rng):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]], F)


PRM = ocr.params(origin=(-2.0, -1.5, -1.0), resolution=0.25, nx=19, ny=13, nz=9, min_range=0.3, max_range=4.0)


def test_random_rays_inside_and_outside(emu):
    rng = np.random.default_rng(21)
    views = []
    # sensor inside; outside on every side (rays enter, miss, or leave at once); returns beyond max_range and below min_range
    for t in ((0.1, 0.2, 0.3), (-3.3, 0.0, 0.1), (3.9, 2.7, 0.0), (0.0, 0.0, 2.1), (0.0, 0.0, -1.9), (2.749, 1.749, 1.249)):
        d = rng.normal(size=(400, 3))
        d /= np.linalg.norm(d, axis=1)[:, None]
        views.append((_rot(rng), np.array(t, F), (d * rng.uniform(0.1, 6.0, (400, 1))).astype(F)))
    L, per_view = _hold(emu, PRM, views)
    assert np.isnan(L).any() and (L > 0).any() and (L < 0).any()
    assert all(int(s[1]) > 0 for s, _, _ in per_view)   # (every view had cut rays)


def test_degenerate_rays(emu):
    Id = np.eye(3, dtype=F)
    t = np.array([0.125, 0.125, 0.125], F)   # a voxel's centre: (8, 6, 4) + 0.5
    ax = [(sgn * r * np.eye(3)[a]) for a in range(3) for sgn in (1, -1) for r in (0.5, 1.0, 3.0, 5.0)]
    diag = [np.array([sx, sy, sz]) * r for sx in (1, -1) for sy in (1, -1) for sz in (1, -1) for r in (0.25, 0.75, 1.0, 2.5)]
    plane = [np.array([r, -r, 0.0]) for r in (0.5, 1.5)] + [np.array([0.0, r, r]) for r in (0.5, 1.5)]
    _hold(emu, PRM, [(Id, t, np.array(ax + diag + plane, F))])
    # from a lattice corner, and from a boundary moving down (n = 0)
    _hold(emu, PRM, [(Id, np.array([0.0, 0.0, 0.0], F), np.array(ax + diag + plane, F))])
    _hold(emu, PRM, [(Id, np.array([0.25, 0.1, 0.1], F), np.array([[-1.0, 0.01, 0.0], [-0.4, -0.4, -0.4]], F))])
    # a return in the sensor's own voxel (zero steps: hit wins over the free of the other rays), non-finite returns, an empty
    # view, a view with non-finite t and one with t too far
    pts = np.array([[0.3, 0.01, 0.0], [1.0, 0.0, 0.0], [np.nan, 0, 0], [0, -np.inf, 0], [0.05, 0, 0]], F)
    PR = dict(PRM, resolution=1.0, origin=(-4.0, -4.0, -4.0), nx=8, ny=8, nz=8)
    L, per_view = _hold(emu, PR, [(Id, np.array([0.2, 0.2, 0.2], F), pts), (Id, t, np.zeros((0, 3), F)),
                                  (Id, np.array([np.nan, 0, 0], F), pts), (Id, np.array([9000.0, 0, 0], F), pts)])
    assert L[4, 4, 4] == F(0.85) and L[4, 4, 5] == F(0.85) and np.isnan(L).sum() == 8 ** 3 - 2
    assert [list(s) for s, _, _ in per_view] == [[2, 0, 0, 2], [0, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0]]


def test_clamping_and_hit_over_free(emu):
    Id = np.eye(3, dtype=F)
    t = np.array([0.125, 0.125, 0.125], F)
    # the second ray crosses the voxel the first one hits: l_hit only
    view = (Id, t, np.array([[1.0, 0, 0], [2.0, 0, 0]], F))
    L, _ = _hold(emu, PRM, [view])
    i, j, k = 8, 6, 4
    assert L[k, j, i + 4] == F(0.85) and L[k, j, i + 8] == F(0.85) and L[k, j, i + 3] == F(-0.4) and L[k, j, i] == F(-0.4)
    L, _ = _hold(emu, PRM, [view] * 12)
    assert L[k, j, i + 4] == F(3.5) and L[k, j, i + 3] == F(-2.0)
    # free then hit then free: the order of the views shows
    L, _ = _hold(emu, PRM, [view, (Id, t, np.array([[0.75, 0, 0]], F)), view])
    assert L[k, j, i + 3] == F(F(F(-0.4) + F(0.85)) + F(-0.4))


def test_tiny_grids_and_word_tails(emu):
    rng = np.random.default_rng(8)
    for nx, ny, nz in ((33, 3, 2), (31, 2, 3), (1, 5, 4), (1, 1, 1)):
        prm = ocr.params(origin=(0.0, 0.0, 0.0), resolution=0.5, nx=nx, ny=ny, nz=nz, min_range=0.05, max_range=10.0)
        hi = np.array([nx, ny, nz]) * 0.5
        for t in (hi * 0.5, hi + 0.7, -hi * 0.3 - 0.2):
            ends = rng.uniform(-1.0, 1.0, (300, 3)) * (hi + 2.0) + hi * 0.5
            _hold(emu, prm, [(np.eye(3, dtype=F), t.astype(F), (ends - t).astype(F))])


def test_limits_are_refused(emu):
    per_view, L = emu(PRM, [])
    assert per_view == [] and np.isnan(L).all()
    bad = [dict(nx=0), dict(ny=1025), dict(nz=0), dict(nx=1024, ny=1024, nz=257), dict(resolution=0.0), dict(resolution=np.inf),
           dict(max_range=0.25 * 4096 * 1.01), dict(min_range=0.0), dict(min_range=5.0), dict(l_hit=-0.1), dict(l_miss=0.0), dict(l_min=0.5),
           dict(l_max=0.0), dict(l_occ=-0.5), dict(l_hit=np.nan), dict(origin=(np.nan, 0.0, 0.0))]
    for kw in bad:
        out = emu(dict(PRM, **kw), [])
        assert isinstance(out, str) and out.startswith("params bad"), kw
    assert not isinstance(emu(dict(PRM, max_range=0.25 * 4096), []), str)   # (exactly 4096 voxels of range: allowed)
