"""tests/tsdf_ray_ref.py is a sensible caster: on surfaces whose truth is known its depth is right to a fraction of a voxel and its
normals to a few degrees.  The bounds are the reference's own measured maxima (include/limovelo_hip.h "Surface ray casting";
DESIGN.md "Surface ray casting" quotes them) rounded up, the depth's to the next multiple of 16 sub-units, the angle's to the next
whole degree, and each is held below the ceiling a caster of this kind must keep: an eighth of a voxel on the finely scanned sphere,
one voxel on the coarsely scanned wall, 15 degrees."""
import numpy as np

import tsdf_cases as tc
import tsdf_ray_cases as cases
import tsdf_ray_ref as trr

F = np.float32
SPHERE_BOUND = 16      # measured -10 .. +5 sub-units
WALL_BOUND = 144       # measured -112 .. +143.5 sub-units
NORMAL_BOUND = 9.0     # measured at most 8.1 degrees (mean 4.1)


def _unit(seed, n):
    d = np.random.default_rng(seed).normal(size=(n, 3))
    return d / np.linalg.norm(d, axis=1)[:, None]


def _sphere(seed, n):
    case = tc.sphere_case(**tc.SPHERE_SMALL)
    ref, prm = tc.reference(case), case["prm"]
    t = (np.asarray(prm["origin"], np.float64) + case["centre"] * prm["resolution"]).astype(F)
    d = _unit(seed, n)
    to = (t.astype(np.float64) + 1.6 * case["radius"] * prm["resolution"] * d).astype(F)
    return case, d, trr.raycast(prm, ref["S"], ref["W"], np.tile(t, (n, 1)), to)


def test_sphere_depth_is_the_radius():
    case, _, (res, _, _) = _sphere(1, 4000)
    assert np.all(res["status"] == trr.HIT)
    err = res["depth"].astype(np.int64) - int(case["radius"] * 256)
    print("sphere depth error, sub-units:", err.min(), err.max())
    assert SPHERE_BOUND % 16 == 0 and SPHERE_BOUND <= 32
    assert np.abs(err).max() <= SPHERE_BOUND


def test_wall_depth_is_the_plane():
    assert WALL_BOUND % 16 == 0 and WALL_BOUND < 256
    seen = 0
    for case in tc.cases():
        if "maxweight4" not in case["name"]:
            continue
        seen += 1
        ref, prm = tc.reference(case), case["prm"]
        rng = np.random.default_rng(5)
        n = 1500
        frm = np.tile(np.asarray(tc.INSIDE, F), (n, 1))
        to = np.stack([np.full(n, 3.4), rng.uniform(-0.3, 3.4, n), rng.uniform(-0.1, 1.8, n)], axis=1).astype(F)
        res, _, _ = trr.raycast(prm, ref["S"], ref["W"], frm, to, case["min_weight"])
        assert np.all(res["status"] == trr.HIT)
        d = to.astype(np.float64) - frm
        d /= np.linalg.norm(d, axis=1)[:, None]
        truth = (2.1 - float(frm[0, 0])) / d[:, 0] / prm["resolution"] * 256.0   # the plane x = 2.1 m
        err = res["depth"] - truth
        print(case["name"], "wall depth error, sub-units:", err.min(), err.max())
        assert np.abs(err).max() <= WALL_BOUND
    assert seen == 2


def test_sphere_normals_point_at_the_sensor():
    _, d, (res, nrm, _) = _sphere(2, 2000)
    assert np.all(res["status"] == trr.HIT)
    assert np.all(nrm.any(axis=1))                                  # none invalid
    length = np.linalg.norm(nrm.astype(np.float64), axis=1)
    assert np.abs(length - 1.0).max() < 1e-6
    # the sensor stood at the centre: outside is towards it
    angle = np.degrees(np.arccos(np.clip(np.sum(nrm.astype(np.float64) * -d, axis=1), -1.0, 1.0)))
    print("sphere normal error, degrees: max", angle.max(), "mean", angle.mean())
    assert NORMAL_BOUND == np.ceil(NORMAL_BOUND) and NORMAL_BOUND < 15.0
    assert angle.max() <= NORMAL_BOUND


def test_metres_follow_the_status():
    c = cases.case("dense-21x4x3")
    res, _, _ = cases.all_answers(c, 1)
    m = trr.metres(c["prm"], res)
    assert np.all(np.isinf(m[res["status"] == trr.CLEAR])) and np.all(np.isnan(m[res["status"] == trr.IGNORED]))
    stop = (res["status"] == trr.HIT) | (res["status"] == trr.BLOCKED)
    assert np.array_equal(m[stop], (F(0.25) * (res["depth"][stop].astype(F) / F(256.0))).astype(F))


def test_the_cases_reach_every_branch():
    for c in cases.cases():
        for mw in c["min_weights"]:
            ans = cases.answers(c["name"], mw)
            res = np.concatenate([ans[n][0] for n in sorted(ans)])
            for status in (trr.IGNORED, trr.CLEAR, trr.HIT, trr.BLOCKED):
                assert (res["status"] == status).any(), (c["name"], mw, status)
            assert ((res["status"] == trr.BLOCKED) & (res["steps"] > 0)).any()       # the back of a surface, or out of unobserved space
            s0 = ans["start_in"][0]
            if mw != c["min_weights"][0] or "shift" in c:   # (the rays were drawn for the first one, and for the box before the recentre)
                continue
            assert np.all(s0["status"] == trr.BLOCKED) and np.all(s0["steps"] == 0) and np.all(s0["axis"] == -1) and np.all(s0["depth"] == 0)
            ig = ans["ignored"][0]
            assert list(ig["status"][:7]) == [0] * 7 and ig["status"][7] != 0 and np.all(ig["cell"][:7] == -1)
            assert all(np.all(ig[f][:7] == 0) for f in trr.RESULT_FIELDS if f != "cell")
            same = ans["from_is_to"][0]
            assert np.all(same["steps"] == 0) and list(same["status"][:2]) == [trr.CLEAR, trr.CLEAR] and list(same["cell"][:2]) == [-1, -1]
            assert same["status"][2] == trr.BLOCKED
            hit = res["status"] == trr.HIT
            assert np.all((res["t"][hit] >= 0) & (res["t"][hit] <= 256)) and np.all(res["t"][~hit & (res["status"] != 0)] == -1)
            assert np.all(res["depth"] >= 0)
    # what the hand-made row is there for
    one, two = cases.answers("long-1024x3x2", 1)["marked"][0], cases.answers("long-1024x3x2", 2)["marked"][0]
    assert list(one["status"]) == [trr.HIT] * 3 and list(one["t"][[0, 2]]) == [0, 0] and one["depth"][0] == 512 and one["depth"][2] == 0
    assert list(two["status"]) == [trr.BLOCKED] * 3 and np.array_equal(two["cell"], one["cell"])
    along = cases.answers("long-1024x3x2", 1)["along_x"][0]
    full = along[:12][along[:12]["status"] == trr.CLEAR]    # the first twelve run from end to end of a row
    assert len(full) == 4 and np.all(full["n_known"] + full["n_unknown"] == 1024)
    # a recentred volume shows the same world: a ray inside both boxes stops in the same voxel of the world
    a, b = cases.case(cases.SOURCES[0]), cases.case(cases.SOURCES[0] + "-recentred")
    assert all(a["rays"][k] is b["rays"][k] for k in a["rays"])
    ra, rb = cases.all_answers(a, 1)[0], cases.all_answers(b, 1)[0]
    both = (ra["status"] == trr.HIT) & (rb["status"] == trr.HIT) & (ra["steps"] == rb["steps"])
    assert both.sum() > 10
    nx, ny = a["prm"]["nx"], a["prm"]["ny"]
    moved = ra["cell"][both] - ((cases.SHIFT[2] * ny + cases.SHIFT[1]) * nx + cases.SHIFT[0])
    assert np.array_equal(moved, rb["cell"][both]) and np.array_equal(ra["depth"][both], rb["depth"][both])
