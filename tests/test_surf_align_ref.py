"""tests/surf_align_ref.py (the rule of "Surface registration" in numpy) against itself: the sample on a field it must reproduce
exactly, its gradient against finite differences, the loop on the scenes of tests/surf_align_cases.py.  No GPU, no library."""
import numpy as np
import pytest

import surf_align_cases as cases
import surf_align_ref as sr


def test_sample_reproduces_a_linear_field():
    """S linear in the voxel index, W = 1, fractions that are multiples of 1/256: every product is exact, so d and n are the
    field and its gradient bit for bit"""
    vol = cases.linear_volume()
    pts, u = cases.exact_points(np.random.default_rng(1), 2000)
    d, n, status = sr.sample(vol, pts.astype(np.float64))
    assert np.all(status == sr.KNOWN) and (u == np.floor(u)).all(axis=1).sum() >= 500
    want = (u @ np.array(cases.LINEAR_COEF, float) + cases.LINEAR_OFFSET) * (cases.LINEAR["resolution"] / 256.0)
    assert np.array_equal(d, want)
    assert np.array_equal(n, np.broadcast_to(np.array(cases.LINEAR_COEF, float) / 256.0, n.shape))


def test_sample_states():
    vol = cases.volume()
    pts = cases.sample_points(np.random.default_rng(2)).astype(np.float64)
    d, n, status = sr.sample(vol, pts)
    assert (np.bincount(status, minlength=3) >= 300).all()              # every state occurs, often
    assert not d[status != sr.KNOWN].any() and not n[status != sr.KNOWN].any()
    assert np.all(status[~np.isfinite(pts).all(axis=1)] == sr.OUTSIDE)
    assert np.abs(d[status == sr.KNOWN]).max() <= 0.3                    # the band
    _, _, s3 = sr.sample(cases.volume(True), pts, min_weight=3)
    assert ((status == sr.KNOWN) & (s3 == sr.UNKNOWN)).sum() >= 100 and not ((s3 == sr.KNOWN) & (status != sr.KNOWN)).any()


def test_gradient_against_finite_differences():
    """inside a cell the interpolant is a cubic polynomial (trilinear): central differences of step h are off by O(h^2) only
    through the xyz term, which a step along one axis does not see; so they agree to rounding, |d| / h * eps ~ 1e-10"""
    vol = cases.volume()
    rng = np.random.default_rng(3)
    floor, wall_x, wall_y = cases.plane_points(rng, 400)
    x = np.concatenate([floor, wall_x, wall_y]) + rng.normal(0, 0.05, (1200, 3))
    o, r = np.asarray(cases.PARAMS["origin"], np.float32).astype(float), float(np.float32(cases.PARAMS["resolution"]))
    f = ((x - o) / r - 0.5) % 1.0
    h = 1e-6
    x = x[np.all((f > 0.01) & (f < 0.99), axis=1)]                       # the step stays inside the cell
    d, n, status = sr.sample(vol, x)
    ok = status == sr.KNOWN
    assert ok.sum() >= 500
    for a in range(3):
        e = np.zeros(3)
        e[a] = h
        fd = (sr.sample(vol, x + e)[0] - sr.sample(vol, x - e)[0]) / (2 * h)
        assert np.abs(fd - n[:, a])[ok].max() <= 1e-9
    assert 0.5 < np.linalg.norm(n[ok], axis=1).mean() <= 1.0 + 1e-6


def test_corner_converges_to_the_truth():
    """the four near guesses end at one pose within resolution / 64 = 1.5625e-3 m of the truth in translation: the floor of the
    quantisation alone moves each plane by up to one sub-unit, sqrt(3) sub-units in all.  Measured: 1.00e-3 m (the creases, where
    the interpolant of min() rounds the corner, pull it further than the 4.4e-4 of points that keep clear of them)."""
    ref, best = cases.reference("corner")
    c = cases.corner()
    for k, r in enumerate(ref[:4]):
        err = float(np.linalg.norm(r["pose"][:3] - cases.TRUTH[:3]))
        print("corner guess", k, "translation error", err, "accepted", r["accepted"], "rejected", r["rejected"], "n_in", r["n_in"])
        assert r["status"] == sr.CONVERGED and err <= float(np.float32(cases.PARAMS["resolution"])) / 64
        assert sr.pose_distance(r["pose"], ref[0]["pose"]) <= 1e-6
        assert 2 <= r["accepted"] <= 6 and r["rejected"] == 0
    assert ref[4]["status"] == sr.NO_OVERLAP and np.array_equal(ref[4]["pose"], c["guesses"][4]) and ref[4]["cost"] == 0.0 and not ref[4]["info"].any()
    assert best[0] in range(4) and best[1] == ref[best[0]]["n_in"]


@pytest.mark.parametrize("name", list(cases.CASES))
def test_accepted_steps_do_not_raise_the_cost(name):
    ref, _ = cases.reference(name)
    for r in ref:
        costs = np.array(r["costs"])
        assert len(costs) == (r["accepted"] + 1 if r["status"] != sr.NO_OVERLAP else 0)
        assert np.all(costs[1:] <= costs[:-1] + 64 * sr.EPS * np.abs(costs[:-1]))
        if name in ("corner", "huber0") and len(costs):
            assert np.all(np.diff(costs) < 0)                            # every accepted step lowers it


def test_floor_holds_the_pose():
    """only the floor: x, y and the yaw about its normal are unobservable.  Their pivots are tiny or not positive, and the damping
    holds them: no guess runs away, and the cost does not rise"""
    ref, _ = cases.reference("floor")
    c = cases.floor()
    for g, r in zip(c["guesses"], ref):
        assert r["status"] == sr.CONVERGED and r["costs"][-1] <= r["costs"][0]
        assert np.linalg.norm(r["pose"][:3] - g[:3]) <= 0.2 and np.isfinite(r["pose"]).all()
        R = sr.gr.rot(r["pose"][3:])
        x = c["source"][:5].astype(float) @ R.T + r["pose"][:3]
        # what is observable is found: the points lie on the floor, to a tenth of a voxel (the crease points tilt it a little)
        assert np.abs(x[:, 2] + 1.0).max() <= 0.01


def test_order_of_the_sums_does_not_decide():
    """the loop with its sums reversed ends where it ended: what the device's tree sums may move"""
    for name in cases.CASES:
        c = cases.CASES[name]()
        ref, best = cases.reference(name)
        rev, best_r = sr.align(c["vol"], c["source"], c["guesses"], reverse=True, **c["solve"])
        worst = 0.0
        for a, b in zip(ref, rev):
            assert (a["n_in"], a["status"], a["accepted"], a["rejected"]) == (b["n_in"], b["status"], b["accepted"], b["rejected"])
            if a["status"] != sr.NO_OVERLAP:
                worst = max(worst, sr.pose_distance(a["pose"], b["pose"]), abs(a["cost"] - b["cost"]) / a["cost"])
        print(name, "reversed sums: worst pose distance or relative cost", worst)
        assert worst <= 1e-11 and best == best_r
