"""tests/ndt_ref.py against itself on the scenes of tests/ndt_cases.py (no GPU, no library).

Forward versus reversed summation: the loop must not owe its outcome to the order of a sum, or no device could be held to it.
Measured on the committed cases: the two runs end at most 4.4e-16 apart and take the same accepted and rejected steps.

Recovery of the truth from the near guesses, measured (max of |dt| in metres and |Log(R^T R_truth)| in radians, the worst of the
eight guesses): corner-near 5.1e-3, corner-search1 6.9e-3.  The bounds below are twice that: the discretisation error of NDT at
1 m voxels is a property of the rule.  The plane, worst of eight: |dz| 1.1e-3 m, roll and pitch 6.8e-3 rad; x, y and yaw are held by
nothing but the voxels' own spread and drift (yaw by up to 0.21 rad in 30 iterations): they are not asserted."""
import numpy as np
import pytest

import graph_ref as gr
import ndt_cases as cases
import ndt_ref as nr

TRUTH_BOUND = {"corner-near": 2 * 5.1e-3, "corner-search1": 2 * 6.9e-3}
PLANE_DZ, PLANE_TILT = 2 * 1.1e-3, 2 * 6.8e-3


def test_gauss_d2():
    assert nr.gauss_d2(1.0, 0.55) == pytest.approx(0.433, abs=5e-4) and nr.gauss_d2(1.0, 0.55) == nr.D2_DEFAULT


@pytest.mark.parametrize("name", list(cases.ALIGN_CASES))
def test_forward_against_reversed(name):
    f, bf = cases.reference(name)
    r, br = cases.reference(name, True)
    worst = 0.0
    for a, b in zip(f, r):
        worst = max(worst, nr.pose_distance(a["pose"], b["pose"]))
        assert (a["accepted"], a["rejected"], a["status"], a["n_in"]) == (b["accepted"], b["rejected"], b["status"], b["n_in"])
    print(name, "forward against reversed:", worst)
    assert worst <= 1e-10 and bf == br


def test_the_cases_hold_what_the_tests_need():
    far, _ = cases.reference("corner-far")
    assert any(r["rejected"] > 0 for r in far)                                      # a run with rejected steps
    local = [r for r in far if r["status"] == nr.MAX_ITERATIONS and nr.pose_distance(r["pose"], cases.TRUTH) > 0.1]
    assert local and all(r["accepted"] + r["rejected"] == cases.SOLVE["max_iterations"] for r in local)   # a local optimum
    assert any(r["status"] == nr.CONVERGED and nr.pose_distance(r["pose"], cases.TRUTH) < 0.01 for r in far)
    assert all(r["n_in"] > 0 for name in cases.ALIGN_CASES for r in cases.reference(name)[0])


@pytest.mark.parametrize("name", cases.NEAR)
def test_truth_is_recovered_from_the_near_guesses(name):
    res, best = cases.reference(name)
    d = [nr.pose_distance(r["pose"], cases.TRUTH) for r in res]
    print(name, "distance from the truth:", d)
    assert all(r["status"] == nr.CONVERGED for r in res) and max(d) <= TRUTH_BOUND[name]
    assert best[0] == int(np.argmax([r["score"] for r in res]))


def test_plane_observes_its_normal():
    res, _ = cases.reference("plane")
    for r in res:
        d = gr.qlog(gr.qmul(gr.qconj(cases.TRUTH[3:]), r["pose"][3:]))
        assert abs(r["pose"][2] - cases.TRUTH[2]) <= PLANE_DZ and abs(d[0]) <= PLANE_TILT and abs(d[1]) <= PLANE_TILT, (r["pose"], d)


def _sigma_omega(T):
    used = np.nonzero(T["n"] >= cases.ROOM["min_points"])[0]
    worst = max(np.abs(nr.full3(T["cov"][c]) @ nr.full3(T["icov"][c]) - np.eye(3)).max() for c in used)
    return worst, len(used)


@pytest.mark.parametrize("name", list(cases.ALIGN_CASES))
def test_sigma_omega_is_the_identity(name):
    worst, n = _sigma_omega(cases.target(name))
    assert n > 30 and worst <= 1e-9


def test_coincident_points_and_min_points():
    prm, pts = cases.coincident()
    T = nr.build(prm, pts)
    assert nr.stats(T) == [9, 0, 1, 1]
    c = int(np.nonzero(T["n"] == 5)[0][0])
    u = 1.0 / 256.0
    assert np.allclose(nr.full3(T["cov"][c]), np.eye(3) * u * u / 12.0, rtol=1e-12, atol=0)   # the quantisation's variance alone
    assert np.abs(T["mean"][c] - pts[0].astype(float)).max() <= u / 2 and _sigma_omega(T)[0] <= 1e-9
    s = int(np.nonzero(T["n"] == 4)[0][0])
    assert not T["mean"][s].any() and not T["cov"][s].any() and not T["icov"][s].any()


def test_dirty_cloud():
    prm, pts = cases.dirty()
    T = nr.build(prm, pts)
    # of the 13 face points, 7.0 / 7.0 / 3.5 lie outside (3); of the 7 bad ones, all
    assert nr.stats(T)[:2] == [500 + 10, 10] and T["n"].sum() == 510
    ok, c, r = nr.voxel_of(prm, np.array([[2.0, 3.0, 0.5], [-1.0, -1.0, -0.5], [np.nextafter(np.float32(7.0), np.float32(0)), 2.0, 1.0]], np.float32))
    assert ok.all() and c.tolist() == [[3, 4, 1], [0, 0, 0], [7, 3, 1]] and r[0].tolist() == [0, 0, 0] and r[2, 0] == 255
    rng = np.random.default_rng(3)
    S = nr.build(prm, pts[rng.permutation(len(pts))])
    for k in ("n", "S1", "S2", "mean", "cov", "icov"):
        assert np.array_equal(T[k], S[k]), k   # integer moments: the order of the points does not show
    half = nr.build(prm, pts[:200])
    both = nr.add(prm, half, pts[200:])
    for k in ("n", "S1", "S2", "mean", "cov", "icov"):
        assert np.array_equal(T[k], both[k]), k
