"""CPU tests of the submap merge's rule as tests/surf_merge_ref.py states it (include/limovelo_hip.h "Submap merging"): what the
rule promises on one lattice, on a linear field and under a change of order, and that every generated case of
tests/surf_merge_cases.py exercises what it claims.  The device and the host emulator are held to the same reference by equality
(tests/test_gpu_surf_merge.py, tests/test_surf_merge_host.py)."""
import numpy as np
import pytest

import surf_merge_cases as mc
import surf_merge_ref as mr

I = np.int64
CASES = mc.cases()


@pytest.fixture(scope="module")
def results():
    return {n: mr.merge(c["dest"], c["sub"], c["pose"], c["min_weight"], c["interp"]) for n, c in CASES.items()}


@pytest.mark.parametrize("name", ["identity", "identity_nearest", "shift", "shift_nearest"])
def test_same_lattice_reproduces_the_source(results, name):
    """At the identity and at whole-voxel translations on one lattice with equal resolution both interpolations give dW == W and
    |dS - S| <= 1 + W / 256 on every known source voxel (step 5's floor: a = floor(256 S / W), dS = floor(a W / 256))."""
    c, r = CASES[name], results[name]
    sub = c["sub"]
    assert r["kq"] == 4096 and all((f[r["state"] != mr.OUTSIDE] == 0).all() for f in r["f"])
    known = r["state"] == mr.KNOWN
    i = [v[known] for v in r["i"]]
    Ss, Ws = sub["S"].astype(I)[i[2], i[1], i[0]], sub["W"].astype(I)[i[2], i[1], i[0]]
    assert known.sum() == (sub["W"] >= 1).sum() and len(set(zip(*i))) == known.sum()   # every known source voxel, once
    assert np.array_equal(r["dW"][known], Ws)
    err = np.abs(r["dS"][known] - Ss)
    assert np.all(256 * err <= 256 + Ws), int(err.max())
    assert not r["dropped"].any() and not r["clamped"].any()
    assert np.array_equal(r["W"][known], Ws.astype(np.int32))   # (into an empty volume the fold adds)


def test_linear_field_within_the_derived_bound():
    """A plane's distance with varying W, turned by 0.6 rad about a skew axis, resolution 0.25 into 0.2: inside both bands dS / dW
    stays within (4 sqrt(3) + 2) * ratio + 2 destination sub-units of the analytic value: the 1/64-voxel position rounding per axis
    (sqrt(3) / 64 source voxels = 4 sqrt(3) source sub-units against a unit gradient), the source's own floor and step 5's (one source
    sub-unit each), and the floors of steps 6 and 7 (one destination sub-unit each)."""
    d, s, pose = mc.linear_field()
    r = mr.merge(d, s, pose)
    ratio = float(s["resolution"]) / float(d["resolution"])
    bound = (4 * np.sqrt(3) + 2) * ratio + 2
    X, Y, Z = (v.astype(np.float64) for v in mr.dr.centres(d["origin"], d["resolution"], d["S"].shape))
    R = mr.rot(pose[1])
    dx = [X - pose[0][0], Y - pose[0][1], Z - pose[0][2]]
    xs = [R[0, b] * dx[0] + R[1, b] * dx[1] + R[2, b] * dx[2] for b in range(3)]
    phi = sum(s["normal"][b] * xs[b] for b in range(3)) - s["offset"]   # metres
    want = phi / float(d["resolution"]) * 256.0
    Ts = s["trunc_cells"] * float(s["resolution"]) - np.sqrt(3) * float(s["resolution"])   # every corner inside the source's band
    Td = d["trunc_cells"] * float(d["resolution"])
    judge = (r["dW"] > 0) & (np.abs(phi) < min(Ts, Td) - 0.05)
    assert judge.sum() > 500 and len(np.unique(r["dW"][judge])) > 10
    err = np.abs(r["dS"][judge] / r["dW"][judge] - want[judge])
    print("linear field: max error %.2f destination sub-units against the bound %.2f over %d voxels" % (err.max(), bound, judge.sum()))
    assert err.max() <= bound


def test_a_weighted_mean_would_not_reproduce_a_linear_field():
    """Why step 5 interpolates the distances unweighted by W: on the linear field above, sum(w S_c) / sum(w W_c), the W-weighted mean of
    the corners' distances, is pulled towards the heavy corners and misses the analytic value by tens of sub-units where the rule stays
    within its bound."""
    d, s, pose = mc.linear_field()
    r = mr.merge(d, s, pose)
    S, W = s["S"].astype(I), s["W"].astype(I)
    known = r["state"] == mr.KNOWN
    num, den = np.zeros(known.shape), np.zeros(known.shape)
    for k in range(8):
        o = (k & 1, (k >> 1) & 1, k >> 2)
        w = np.ones(known.shape, I)
        for b in range(3):
            w = w * (r["f"][b] if o[b] else mr.FR - r["f"][b])
        idx = [np.where(known & (w != 0), r["i"][b] + o[b], 0) for b in range(3)]
        num += w * S[idx[2], idx[1], idx[0]]
        den += w * W[idx[2], idx[1], idx[0]]
    X, Y, Z = (v.astype(np.float64) for v in mr.dr.centres(d["origin"], d["resolution"], d["S"].shape))
    R = mr.rot(pose[1])
    dx = [X - pose[0][0], Y - pose[0][1], Z - pose[0][2]]
    phi = sum(s["normal"][b] * (R[0, b] * dx[0] + R[1, b] * dx[1] + R[2, b] * dx[2]) for b in range(3)) - s["offset"]
    judge = (r["dW"] > 0) & (np.abs(phi) < 1.4)   # (inside both bands of 2 m and 1.6 m with every corner)
    ratio = float(s["resolution"]) / float(d["resolution"])
    want = phi[judge] / float(d["resolution"]) * 256.0
    weighted = np.abs(num[judge] / den[judge] * ratio - want)
    ruled = np.abs(r["dS"][judge] / r["dW"][judge] - want)
    print("W-weighted mean: max error %.1f destination sub-units, the rule %.1f, over %d voxels" % (weighted.max(), ruled.max(), judge.sum()))
    assert ruled.max() <= (4 * np.sqrt(3) + 2) * ratio + 2 and weighted.max() > 5 * ruled.max()


def test_order_does_not_matter_below_max_weight():
    d, subs = mc.pair()
    ab = mr.merged(d, mr.merge(d, *subs[0]))
    ab = mr.merged(ab, mr.merge(ab, *subs[1]))
    ba = mr.merged(d, mr.merge(d, *subs[1]))
    ba = mr.merged(ba, mr.merge(ba, *subs[0]))
    both = (mr.merge(d, *subs[0])["dW"] > 0) & (mr.merge(d, *subs[1])["dW"] > 0)
    assert both.sum() > 200 and ab["W"].max() < d["max_weight"]
    assert np.array_equal(ab["S"], ba["S"]) and np.array_equal(ab["W"], ba["W"])


@pytest.mark.parametrize("name", list(CASES))
def test_case_exercises_what_it_claims(results, name):
    c, r = CASES[name], results[name]
    st = r["state"]
    n = c["sub"]["S"].shape[::-1]
    last = np.zeros(st.shape, bool)
    for b in range(3):
        last |= (st != mr.OUTSIDE) & (r["f"][b] == 0) & (r["i"][b] == n[b] - 1)
    box = mr.box_voxels(c["dest"], c["sub"], c["pose"])   # the voxels the call is launched over: the issue's destination box
    print(f"{name}: {int((r['dW'] > 0).sum())} of a box of {box} voxels contribute")
    seen = {"quarter": 4 * int((r["dW"] > 0).sum()) >= box > 0, "outside": (st == mr.OUTSIDE).any(),
            "unknown": (st == mr.UNKNOWN).any(), "dropped": r["dropped"].any(), "clamped": (r["clamped"] & (r["dW"] > 0)).any(),
            "folded": r["folded"].any(), "last_layer": last.any()}
    for claim in c["claims"]:
        assert seen[claim], f"{name} does not exercise {claim}"
    assert int(r["stats"][0]) == int((st != mr.OUTSIDE).sum()) and int(r["stats"][2]) == int(r["dW"].sum())
    if name == "misses":
        assert not r["stats"].any() and np.array_equal(r["S"], c["dest"]["S"])
    if name == "grazes":
        assert 0 < int(r["stats"][0]) < 200
    if name == "min_weight":
        assert (mr.merge(c["dest"], c["sub"], c["pose"], 1)["dW"] > 0).sum() > (r["dW"] > 0).sum() > 0


def test_every_claim_is_exercised_by_some_case():
    assert set().union(*(c["claims"] for c in CASES.values())) == {"quarter", "outside", "unknown", "dropped", "clamped", "folded", "last_layer"}


def test_scale():
    assert mr.scale(0.2, 0.2) == 4096 and mr.scale(0.25, 0.2) == 5120 and mr.scale(0.1, 0.2) == 2048
    assert mr.scale(0.025, 0.2) == 512 and mr.scale(1.6, 0.2) == 32768
    assert mr.scale(0.0249, 0.2) is None and mr.scale(1.61, 0.2) is None
