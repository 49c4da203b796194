"""CPU tests of the aiding observations' reference and host helpers.

tests/aiding_ref.py (f64, the stated summation order) is what tests/test_gpu_observe.py holds the device to at 1e-12.  Here it is
anchored, on every case of tests/aiding_cases.py, to a 50-digit restatement of the same rule written differently: a dense
3 x 23 H, S^-1 by mpmath's inverse, K = P H^T S^-1 and the Joseph form as whole-matrix products, the manifold parts from
tests/manifold_mp.py.  The two share no code beyond the case table, so the comparison checks the rule as well as its rounding.
The largest difference is printed and must lie two decades under the device's bounds (1e-14); S must be well conditioned
(<= 1e3) wherever an observation is applied, so a device that misses 1e-12 is wrong, not unlucky."""
import mpmath as mp
import numpy as np
import pytest

import aiding_cases as ac
import aiding_ref as ar
import manifold_mp as mm

ANCHOR = 1e-14      # two decades under the 1e-12 of tests/test_gpu_observe.py
COND_MAX = 1e3


@pytest.fixture(scope="module")
def aiding(lv):
    from limo_velo_amd import aiding as a

    return a


def _mpv(a):
    return [mp.mpf(float(t)) for t in np.ravel(a)]


def boxplus_mp(x, d):
    o = list(x)
    for i in range(3):
        o[i] = x[i] + d[i]
    o[3:7] = mm.quat_mul(x[3:7], mm.so3_exp(d[3:6]))
    o[7:11] = mm.quat_mul(x[7:11], mm.so3_exp(d[6:9]))
    for s, t in ((11, 9), (14, 12), (17, 15), (20, 18)):
        for i in range(3):
            o[s + i] = x[s + i] + d[t + i]
    o[23:26] = mm.s2_boxplus(x[23:26], d[21:23])
    return o


def observe_mp(x, P, o):
    """x: 26 mpf, P: mp.matrix 23 x 23 -> x, P, status, nis, y (3 mpf), S (mp.matrix or None)."""
    z, lever = _mpv(o["z"]), _mpv(o["lever"])
    R = mp.matrix(mm.quat_to_rot(x[3:7]))
    H = mp.zeros(3, 23)
    if o["kind"] == ac.POSITION:
        h = mp.matrix(x[0:3]) + R * mp.matrix(lever)
        y = mp.matrix(z[:3]) - h
        H[0:3, 0:3] = mp.eye(3)
        H[0:3, 3:6] = -(R * mp.matrix(mm.hat(lever)))
    elif o["kind"] == ac.VELOCITY_WORLD:
        y = mp.matrix(z[:3]) - mp.matrix(x[14:17])
        H[0:3, 12:15] = mp.eye(3)
    elif o["kind"] == ac.VELOCITY_BODY:
        vb = R.T * mp.matrix(x[14:17])
        y = mp.matrix(z[:3]) - vb
        H[0:3, 12:15] = R.T
        H[0:3, 3:6] = mp.matrix(mm.hat(list(vb)))
    else:
        conj = [-x[3], -x[4], -x[5], x[6]]
        y = mp.matrix(mm.so3_log(mm.quat_mul(conj, z)))
        H[0:3, 3:6] = mp.eye(3)
    comp = [k for k in range(3) if o["mask"] >> k & 1]
    m = len(comp)
    Hm = mp.matrix([[H[k, c] for c in range(23)] for k in comp])
    ym = mp.matrix([y[k] for k in comp])
    Rf = np.asarray(o["R"], np.float64).reshape(3, 3)
    Rm = mp.matrix([[mp.mpf(float(Rf[a, b])) for b in comp] for a in comp])
    S = Hm * P * Hm.T + Rm
    y3 = [y[k] for k in range(3)]
    if any(mp.det(S[0:k, 0:k]) <= 0 for k in range(1, m + 1)):   # not positive definite
        return x, P, 2, mp.mpf(0), y3, None
    Si = S ** -1
    nis = (ym.T * Si * ym)[0]
    if o["gate"] > 0 and nis > mp.mpf(o["gate"]):
        return x, P, 1, nis, y3, S
    K = P * Hm.T * Si
    dx = K * ym
    A = mp.eye(23) - K * Hm
    Pn = A * P * A.T + K * Rm * K.T
    return boxplus_mp(x, list(dx)), Pn, 0, nis, y3, S


def _err(a, b_mp):
    return float(max(abs(mp.mpf(float(s)) - t) for s, t in zip(np.ravel(a), b_mp)))


@pytest.fixture(scope="module")
def runs(oracle):
    """Every case through the f64 reference: computed once, shared."""
    return {c["name"]: ar.observe(oracle, c["x"], c["P"], c["obs"]) for c in ac.cases()}


def test_table_holds_the_required_cases(runs):
    table = {c["name"]: c for c in ac.cases()}
    kinds = {o["kind"] for c in table.values() for o in c["obs"]}
    assert kinds == {1, 2, 3, 4}
    assert {c["obs"][0]["mask"] for c in table.values() if c["obs"][0]["kind"] == ac.POSITION} == set(range(1, 8))
    levers = [np.any(o["lever"] != 0) for c in table.values() for o in c["obs"] if o["kind"] == ac.POSITION]
    assert any(levers) and not all(levers)
    for angle in (0.01, 0.3, 3.0):
        for kind in ac.KIND_NAMES.values():
            c = table[f"{kind}-rot{angle}"]
            w = c["x"][6]
            assert abs(2 * np.arccos(w) - angle) < 1e-9
    # gravity beside the pole of its chart (the regular branch of the basis, a small denominator) and at it (the other branch)
    assert 0 < table["grav-beside-pole"]["x"][23] + ac.S2_LEN < 1e-6 and table["grav-at-pole"]["x"][23] + ac.S2_LEN == 0
    # the exponential's small-angle branch is below |d| = 2 * 2^-6.5 = 0.0221: both sides are taken
    rot = {n: np.linalg.norm(r[2][0]["dx"][3:6]) for n, r in runs.items() if r[2][0]["status"] == 0}
    assert rot["attitude-large"] > 0.0222 and min(rot.values()) < 0.0221
    assert [r["status"] for r in runs["gated"][2]] == [1]
    assert [r["status"] for r in runs["singular"][2]] == [2]
    assert not table["singular"]["P"].any() and not table["singular"]["obs"][0]["R"].any()
    assert [r["status"] for r in runs["batch8"][2]] == [0, 0, 1, 0, 0, 0, 0, 0] and len(table["batch8"]["obs"]) == 8
    for name, (x, P, res) in runs.items():
        if ac.applied(table[name]):
            assert [r["status"] for r in res] == [0], name
            # every block of the state moves: the dense P couples the observation to all of it
            d = np.abs(x - table[name]["x"])
            assert all(d[s].max() > 1e-6 for s in (slice(0, 3), slice(3, 7), slice(7, 11), slice(14, 17), slice(23, 26))), name
        else:   # untouched by status 1 and 2
            for r, o in zip(res, table[name]["obs"]):
                assert r["rows"] == bin(o["mask"]).count("1")
    x, P, _ = runs["gated"]
    assert np.array_equal(x, table["gated"]["x"]) and np.array_equal(P, table["gated"]["P"])
    x, P, _ = runs["singular"]
    assert np.array_equal(x, table["singular"]["x"]) and np.array_equal(P, table["singular"]["P"])


def test_reference_against_50_digits(oracle, runs):
    worst = dict(x=0.0, P=0.0, nis=0.0, y=0.0, cond=0.0)
    where = {}
    for c in ac.cases():
        xr, Pr = np.array(c["x"]), np.array(c["P"])
        xm, Pm = _mpv(c["x"]), mp.matrix([[mp.mpf(float(t)) for t in row] for row in c["P"]])
        for k, o in enumerate(c["obs"]):
            xr, Pr, r = ar.observe_one(oracle, xr, Pr, o)
            xm, Pm, status, nis, y3, S = observe_mp(xm, Pm, o)
            assert r["status"] == status, (c["name"], k)
            e = dict(x=_err(xr, xm), P=_err(Pr, list(Pm)) / max(1.0, float(np.abs(Pr).max())),
                     nis=abs(r["nis"] - float(nis)) / max(1.0, float(nis)) if status != 2 else 0.0, y=_err(r["y"], y3))
            if status == 0:
                ev = np.linalg.eigvalsh(np.array([[float(S[a, b]) for b in range(S.cols)] for a in range(S.rows)]))
                e["cond"] = float(ev[-1] / ev[0])
                assert e["cond"] <= COND_MAX, (c["name"], k, e["cond"])
                assert np.array_equal(Pr, Pr.T)
            for key, v in e.items():
                if v > worst[key]:
                    worst[key], where[key] = v, (c["name"], k)
        assert np.array_equal(xr, runs[c["name"]][0]) and np.array_equal(Pr, runs[c["name"]][1])
    print("aiding_ref vs 50 digits, worst: " + ", ".join(f"{k} {v:.3e} at {where.get(k)}" for k, v in worst.items()))
    assert worst["x"] <= ANCHOR and worst["P"] <= ANCHOR and worst["nis"] <= ANCHOR and worst["y"] <= ANCHOR, worst


def test_joseph_form_equals_the_short_form_and_is_symmetric(runs):
    """With the optimal gain the Joseph form equals P - K S K^T: a check of the reference's bookkeeping by a different formula."""
    for c in ac.cases():
        if not ac.applied(c):
            continue
        _, Pn, res = runs[c["name"]]
        o = c["obs"][0]
        comp = ar.components(o["mask"])
        _, blocks = ar.model(c["x"], o)
        H = np.zeros((len(comp), 23))
        for c0, blk in blocks:
            H[:, c0:c0 + 3] = np.array(blk)[comp]
        S = res[0]["S"]
        K = c["P"] @ H.T @ np.linalg.inv(S)
        assert np.abs(Pn - (c["P"] - K @ S @ K.T)).max() < 1e-13, c["name"]
        assert np.linalg.eigvalsh(Pn)[0] > 0


# ---- limo_velo_amd.aiding ------------------------------------------------------------------------------
def test_records(aiding):
    from limo_velo_amd import capi

    o = aiding.position((1, 2, 3), cov=0.25, lever=(0.1, 0, 0.3), gate=aiding.chi2_gate(3, 0.99))
    assert (o.kind, o.mask, list(o.z), list(o.lever), o.gate) == (capi.OBS_POSITION, 7, [1, 2, 3, 0], [0.1, 0, 0.3], 11.344866730144373)
    assert np.array_equal(np.array(o.R[:]).reshape(3, 3), 0.25 * np.eye(3))
    b = aiding.position(12.5, cov=0.04, axes="z")
    assert (b.mask, list(b.z)[:3], b.gate) == (4, [0, 0, 12.5], 0.0) and b.R[8] == 0.04
    w = aiding.body_velocity(3.0, cov=0.01)
    assert (w.kind, w.mask, list(w.z)[:3]) == (capi.OBS_VELOCITY_BODY, 1, [3.0, 0, 0])
    n = aiding.body_velocity((3.0, 0, 0), cov=(0.01, 0.0004, 0.0004), axes="xyz")
    assert n.mask == 7 and [n.R[0], n.R[4], n.R[8]] == [0.01, 0.0004, 0.0004]
    zu = aiding.zupt(1e-4)
    assert (zu.kind, zu.mask, list(zu.z)) == (capi.OBS_VELOCITY_WORLD, 7, [0, 0, 0, 0])
    assert aiding.world_velocity((1, 2), cov=(0.1, 0.2), axes="xy").mask == 3
    a = aiding.attitude((0, 0, 2, 2), cov=1e-3)
    assert a.kind == capi.OBS_ATTITUDE and abs(np.linalg.norm(a.z[:]) - 1) < 1e-15 and a.z[2] == a.z[3]
    full = np.array([[2, 0.1, 0], [0.1, 3, 0.2], [0, 0.2, 4]], float)
    assert np.array_equal(np.array(aiding.position((0, 0, 0), full).R[:]).reshape(3, 3), full)
    for bad in (lambda: aiding.position((1, 2, 3), 1.0, axes="xx"), lambda: aiding.position((1, 2, 3), 1.0, axes=""),
                lambda: aiding.position((1, 2), 1.0), lambda: aiding.position((1, 2, 3), (1, 2)), lambda: aiding.attitude((0, 0, 0, 0), 1.0),
                lambda: aiding.chi2_gate(4, 0.95), lambda: aiding.chi2_gate(2, 0.9)):
        with pytest.raises(ValueError):
            bad()


def test_chi2_gate_table(aiding):
    for rows in (1, 2, 3):
        for p in (0.95, 0.99, 0.999):
            g = aiding.chi2_gate(rows, p)
            assert abs(mp.gammainc(mp.mpf(rows) / 2, 0, mp.mpf(g) / 2, regularized=True) - mp.mpf(p)) < 1e-12, (rows, p)


def test_enu_from_lla(aiding):
    origin = (48.0, 11.0, 500.0)
    assert np.array_equal(aiding.enu_from_lla(*origin, origin), [0, 0, 0])
    # straight up: the ellipsoid's normal
    assert np.abs(aiding.enu_from_lla(48.0, 11.0, 600.0, origin) - [0, 0, 100]).max() < 1e-8
    # one arc-second of latitude at the equator is the meridian's radius of curvature there, a (1 - e^2), times the angle:
    # 6335439.327 m * pi / 648000 = 30.715 m; at 45 degrees M = a (1 - e^2) / (1 - e^2 / 2)^1.5 = 6367381.816 m: 30.870 m
    sec = 1.0 / 3600.0
    e2 = (2 - 1 / 298.257223563) / 298.257223563
    for lat0, M in ((0.0, 6378137.0 * (1 - e2)), (45.0, 6378137.0 * (1 - e2) / (1 - e2 / 2) ** 1.5)):
        d = aiding.enu_from_lla(lat0 + sec / 2, 7.0, 0.0, (lat0 - sec / 2, 7.0, 0.0))
        assert abs(d[1] - M * np.pi / 648000) < 1e-4 and abs(d[0]) < 1e-9 and 30.7 < d[1] < 30.9
    # one arc-second of longitude at latitude 60: N cos(lat) * angle, N = a / sqrt(1 - e^2 sin^2)
    N = 6378137.0 / np.sqrt(1 - e2 * np.sin(np.radians(60.0)) ** 2)
    d = aiding.enu_from_lla(60.0, 7.0 + sec, 0.0, (60.0, 7.0, 0.0))
    assert abs(d[0] - N * 0.5 * np.pi / 648000) < 1e-4 and abs(d[1]) < 1e-3
    arr = aiding.enu_from_lla(np.array([48.0, 48.001]), np.array([11.0, 11.002]), np.array([500.0, 510.0]), origin)
    assert arr.shape == (2, 3) and np.array_equal(arr[0], [0, 0, 0]) and abs(arr[1, 2] - 10) < 0.1


def test_fit_frame_recovers_a_known_frame(aiding):
    rng = np.random.default_rng(5)
    enu = np.c_[np.cumsum(rng.normal(size=(40, 2)), axis=0) * 3, rng.normal(size=40) * 0.2]
    for yaw, t in ((0.7, np.array([12.0, -5.0, 1.5])), (-2.9, np.array([-100.0, 40.0, -3.0])), (np.pi / 2, np.zeros(3))):
        m = aiding.to_map(yaw, t, enu)
        yaw_fit, t_fit = aiding.fit_frame(m, enu)
        assert abs(np.angle(np.exp(1j * (yaw_fit - yaw)))) < 1e-9 and np.abs(t_fit - t).max() < 1e-9
        assert np.abs(aiding.to_map(yaw_fit, t_fit, enu) - m).max() < 1e-9
    with pytest.raises(ValueError):
        aiding.fit_frame(np.zeros((5, 3)), np.zeros((5, 3)))


def test_static_init(aiding):
    # a level sensor, then one rolled and pitched: clean data
    x = aiding.static_init(np.tile([0, 0, 9.809], (50, 1)), np.zeros((50, 3)))
    assert np.array_equal(x[3:7], [0, 0, 0, 1]) and np.array_equal(x[23:26], [0, 0, -9.809]) and not x[17:20].any()
    q = ac.quat_exp([0.2, -0.1, 0.0])                      # body to map
    R = ac.quat_rot(q)
    f = R.T @ np.array([0, 0, 9.809])                      # the specific force the tilted sensor reads at rest
    x = aiding.static_init(np.tile(f, (100, 1)), np.tile([0.001, -0.002, 0.0005], (100, 1)))
    assert abs(np.linalg.norm(x[23:26]) - 9.809) < 1e-12 and abs(np.linalg.norm(x[3:7]) - 1) < 1e-15
    assert np.abs(x[17:20] - [0.001, -0.002, 0.0005]).max() < 1e-15
    Rx = ac.quat_rot(x[3:7])
    assert np.abs(Rx @ f + x[23:26]).max() < 1e-12         # R acc + grav = 0: at rest
    assert np.abs(x[3:7] - q).max() < 1e-12                 # (the tilt had no heading: the smallest rotation is the tilt itself)
    assert np.array_equal(x[7:11], [0, 0, 0, 1]) and not x[0:3].any() and not x[11:17].any() and not x[20:23].any()
    x = aiding.static_init([[0, 0, -9.809]], [[0, 0, 0]])   # upside down
    assert np.abs(ac.quat_rot(x[3:7]) @ np.array([0, 0, -9.809]) + x[23:26]).max() < 1e-12
