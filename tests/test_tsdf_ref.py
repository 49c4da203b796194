"""The TSDF's rule as tests/tsdf_ref.py states it (include/limovelo_hip.h "TSDF and mesh"), checked on its own: a ray worked out by
hand, independence of the order and of the split over views, the max_weight rescale against by-hand values, and the sphere: the
mesh of a sphere scanned from inside lies on the sphere, is closed and oriented towards the sensor.  No GPU."""
import numpy as np

import tsdf_cases as tc
import tsdf_ref as tr

F = np.float32

# 1 m voxels from the origin; the sensor in the centre of voxel (0, 1, 1): qs = (128, 384, 384).  trunc_cells 2: T = 512.
LINE = tr.params(origin=(0.0, 0.0, 0.0), resolution=1.0, nx=12, ny=3, nz=3, min_range=0.5, max_range=11.0, trunc_cells=2)
SENSOR = np.array([0.5, 1.5, 1.5], F)


def _line(prm, S, W, returns):
    return tr.integrate(prm, S, W, [(tc.ID, SENSOR, np.array(returns, F))])


def test_one_ray_along_x_by_hand():
    # the return at 6 m: qe = (1664, 384, 384), d = (1536, 0, 0), len = 1536, ext = (512, 0, 0), qa = 1152 (the centre of voxel 4),
    # qb = 2176 (the centre of voxel 8).  The centres 256 v + 128 of voxels 4..8 give s = 1664 - c = 512, 256, 0, -256, -512.
    S, W, st = _line(LINE, *tr.empty(LINE), [[6.0, 0, 0]])
    assert list(S[1, 1]) == [0, 0, 0, 0, 512, 256, 0, -256, -512, 0, 0, 0]
    assert list(W[1, 1]) == [0, 0, 0, 0, 1, 1, 1, 1, 1, 0, 0, 0]
    assert list(st) == [1, 0, 5, 5] and W.sum() == 5
    m = tr.metres(LINE, S, W)
    assert list(m[1, 1, 4:9]) == [2.0, 1.0, 0.0, -1.0, -2.0] and np.isnan(m[1, 1, 3])
    # carve: the walk starts at the sensor, voxels 0..3 take s = T
    carve = dict(LINE, carve=1)
    S, W, st = _line(carve, *tr.empty(carve), [[6.0, 0, 0]])
    assert list(S[1, 1]) == [512, 512, 512, 512, 512, 256, 0, -256, -512, 0, 0, 0] and list(st) == [1, 0, 9, 9]
    # a CUT return (12 m > max_range: cut to 11 m, qe = 2944 in voxel 11): nothing without carve; with it s = T on voxels 0..11
    S, W, st = _line(LINE, *tr.empty(LINE), [[12.0, 0, 0]])
    assert not W.any() and list(st) == [0, 0, 0, 0]
    S, W, st = _line(carve, *tr.empty(carve), [[12.0, 0, 0]])
    assert list(S[1, 1]) == [512] * 12 and list(W[1, 1]) == [1] * 12 and list(st) == [1, 1, 12, 12]
    # a hit closer than T (1.5 m: len = 384 <= 512): the walk starts at the sensor although carve = 0
    S, W, st = _line(LINE, *tr.empty(LINE), [[1.5, 0, 0]])
    assert list(S[1, 1][:5]) == [384, 128, -128, -384, 0] and list(W[1, 1][:5]) == [1, 1, 1, 1, 0]


def test_order_and_split_change_no_bit():
    rng = np.random.default_rng(5)
    for carve in (0, 1):
        prm = tc.grid_params(33, 17, 9, carve=carve)
        R, t, pts = tc.random_view(rng, tc.INSIDE, 600)
        S0, W0 = tr.empty(prm)
        S0, W0, _ = tr.integrate(prm, S0, W0, [tc.wall_view(tc.INSIDE, 300)])   # (something to fold into)
        S1, W1, st1 = tr.integrate(prm, S0, W0, [(R, t, pts)])
        S2, W2, st2 = tr.integrate(prm, S0, W0, [(R, t, pts[rng.permutation(len(pts))])])
        S3, W3, st3 = tr.integrate(prm, S0, W0, [(R, t, pts[400:]), (R, t, pts[:150]), (R, t, pts[150:400])])
        assert W1.any() and not np.array_equal(S1, S0)
        for S, W, st in ((S2, W2, st2), (S3, W3, st3)):
            assert np.array_equal(S, S1) and np.array_equal(W, W1) and list(st) == list(st1)


def test_max_weight_rescales_by_hand():
    prm = dict(LINE, max_weight=4)
    S, W = tr.empty(prm)
    S, W, _ = _line(prm, S, W, [[6.0, 0, 0]] * 3)
    assert list(S[1, 1, 4:9]) == [1536, 768, 0, -768, -1536] and list(W[1, 1, 4:9]) == [3] * 5
    S, W, st = _line(prm, S, W, [[6.0, 0, 0]] * 3)   # Wn = 6 > 4: S = floor(6 s * 4 / 6) = 4 s
    assert list(S[1, 1, 4:9]) == [2048, 1024, 0, -1024, -2048] and list(W[1, 1, 4:9]) == [4] * 5 and list(st) == [3, 0, 15, 5]
    # one return at 6.3 m: qe = 1740 (0.5 + 6.3 = 6.8000002 in f32, * 256 = 1740.8), len = 1612, ext = 512: voxels 4..8 take
    # s = 1740 - c = 588 -> 512, 332, 76, -180, -436.  Wn = 5 > 4: S = floor((S + s) * 4 / 5):
    # 2560 * 4 / 5 = 2048; 1356 * 4 / 5 = 1084.8 -> 1084; 76 * 4 / 5 = 60.8 -> 60; -1204 * 4 / 5 = -963.2 -> -964;
    # -2484 * 4 / 5 = -1987.2 -> -1988 (floor, not truncation)
    S, W, st = _line(prm, S, W, [[6.3, 0, 0]])
    assert list(S[1, 1, 4:9]) == [2048, 1084, 60, -964, -1988] and list(W[1, 1, 4:9]) == [4] * 5 and list(st) == [1, 0, 5, 5]


def _topology(tri):
    """(every undirected edge in exactly two triangles, every directed edge once, the number of undirected edges)"""
    t = tri.astype(np.int64)
    directed = np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])
    _, dc = np.unique(directed, axis=0, return_counts=True)
    _, uc = np.unique(np.sort(directed, axis=1), axis=0, return_counts=True)
    return bool(np.all(uc == 2)), bool(np.all(dc == 1)), len(uc)


def _signed_volume(v, tri):
    a, b, c = (v[tri[:, i].astype(np.int64)] for i in range(3))
    return float(np.sum(np.einsum("ij,ij->i", a, np.cross(b, c))) / 6.0)


def _check_sphere(spec, vertices=None, triangles=None):
    """The 0.1 voxel is derived, not tuned: quantisation (at most 2 / 256), the off-ray term delta^2 / 2r (at most 0.02), the chord
    sagitta (at most 0.02) and the floors.  Measured: 0.022 voxel at radius 20 (7534 vertices), 0.045 at radius 6."""
    case = tc.sphere_case(**spec)
    ref = tc.reference(case)
    mesh = ref["mesh"]
    counts = [int(c) for c in mesh["counts"]]
    if vertices is not None:
        assert counts == [vertices, triangles, vertices, 0]
    assert counts[3] == 0 and counts[0] > 0
    v = mesh["sub"].astype(np.float64) / 256.0
    err = np.abs(np.linalg.norm(v - case["centre"], axis=1) - case["radius"])
    print(case["name"], "vertices", counts[0], "triangles", counts[1], "largest distance from the sphere (voxels)", err.max())
    assert err.max() <= 0.1
    two, once, E = _topology(mesh["tri"])
    assert two and once
    assert counts[0] - E + counts[1] == 2
    assert _signed_volume(v, mesh["tri"]) < 0     # (the normals point at the sensor)
    # the metres of the vertices, against f64 within f32 rounding
    prm = case["prm"]
    want = np.asarray(prm["origin"], np.float64) + prm["resolution"] * v
    assert np.abs(mesh["xyz"] - want).max() < 1e-5
    assert int(ref["stats"][0][0]) == len(case["calls"][0][0][2])   # (every ray of the pattern was used)


def test_sphere_radius_20():
    _check_sphere(tc.SPHERE_LARGE, 7534, 15064)


def test_sphere_radius_6():
    _check_sphere(tc.SPHERE_SMALL, 680, 1356)
