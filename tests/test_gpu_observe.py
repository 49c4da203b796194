"""Aiding observations on the resident filter (lv_observe, include/limovelo_hip.h "Aiding observations") against the f64
restatement of the rule (tests/aiding_ref.py, anchored to 50 digits by tests/test_aiding_ref.py) on the cases of
tests/aiding_cases.py, and against themselves: a batch equals its observations one by one, the order with queued predictions
holds, the result does not depend on where the filter was, and what follows (lv_correct, lv_map_add_scan) starts from the
observed state.

Bounds: a single observation |x - x_ref| <= 1e-12 and |P - P_ref| <= 1e-12 max(1, max|P_ref|), the single-step bounds of
lv_predict in tests/test_gpu_filter.py; chains 1e-9 in the same form.  nis and y are held to 1e-12 max(1, |ref|): the same
arithmetic on S, whose condition the case table keeps below 1e3 (measured 2.6)."""
import ctypes as C

import numpy as np
import pytest

import aiding_cases as ac
import aiding_ref as ar

pytestmark = pytest.mark.gpu

TOL_ONE = 1e-12
TOL_STATE = 1e-9


def _Q():
    return np.diag([1e-4] * 3 + [1e-2] * 3 + [1e-5] * 3 + [1e-4] * 3)


@pytest.fixture(scope="module")
def capi(lv):
    from limo_velo_amd import capi as c

    return c


@pytest.fixture(scope="module")
def refs(oracle):
    """Every case through the reference: computed once, shared, never changed."""
    return {c["name"]: ar.observe(oracle, c["x"], c["P"], c["obs"]) for c in ac.cases()}


def _rec(capi, o):
    return capi.default_observation(o["kind"], mask=o["mask"], z=o["z"], R=o["R"], lever=o["lever"], gate=o["gate"])


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _same(a, b):
    return np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(_bits(a[1]), _bits(b[1]))


def _within(x, P, xr, Pr, tol, what):
    ex, eP = np.abs(x - xr).max(), np.abs(P - Pr).max() / max(1.0, np.abs(Pr).max())
    print(f"{what}: |x - ref| {ex:.3e}, |P - ref| / max(1, max|P|) {eP:.3e}")
    assert ex <= tol and eP <= tol, (what, ex, eP)


def _invariants(x, P, what):
    assert np.array_equal(_bits(P), _bits(P.T)), what                      # exactly symmetric
    assert abs(np.linalg.norm(x[3:7]) - 1) <= 1e-12 and abs(np.linalg.norm(x[7:11]) - 1) <= 1e-12, what
    assert abs(np.linalg.norm(x[23:26]) - 9.809) <= 1e-9, what


def _results_match(got, want, what):
    assert len(got) == len(want), what
    for k, (g, w) in enumerate(zip(got, want)):
        assert (g["status"], g["rows"]) == (w["status"], w["rows"]), (what, k, g, w)
        assert abs(g["nis"] - w["nis"]) <= TOL_ONE * max(1.0, abs(w["nis"])), (what, k, g["nis"], w["nis"])
        assert np.abs(g["y"] - w["y"]).max() <= TOL_ONE * max(1.0, np.abs(w["y"]).max()), (what, k)
        if w["status"] == 2:
            assert g["nis"] == 0.0


def test_single_observations(capi, refs):
    with capi.Context() as ctx:
        for c in ac.cases():
            if len(c["obs"]) != 1:
                continue
            xr, Pr, rr = refs[c["name"]]
            ctx.filter_set(c["x"], c["P"])
            assert ctx.observe([_rec(capi, c["obs"][0])]) is None
            x, P = ctx.filter_get()
            _results_match(ctx.observe_results(), rr, c["name"])
            _within(x, P, xr, Pr, TOL_ONE, c["name"])
            if rr[0]["status"] == 0:
                _invariants(x, P, c["name"])
                assert not np.array_equal(x, c["x"]) and not np.array_equal(P, c["P"])
            else:   # gated out, S not positive definite: not a bit moves
                assert _same((x, P), (c["x"], c["P"])), c["name"]
        assert {refs[n][2][0]["status"] for n in ("gated", "singular", "wheel")} == {0, 1, 2}


def test_batch_equals_sequence(capi, refs):
    c = next(c for c in ac.cases() if c["name"] == "batch8")
    recs = [_rec(capi, o) for o in c["obs"]]
    xr, Pr, rr = refs["batch8"]
    with capi.Context() as ctx:
        ctx.filter_set(c["x"], c["P"])
        res_batch = ctx.observe(recs, wait=True)
        batch = ctx.filter_get()
        ctx.filter_set(c["x"], c["P"])
        res_seq = []
        for r in recs:
            ctx.observe([r])
            res_seq += ctx.observe_results()
        seq = ctx.filter_get()
    assert _same(batch, seq)
    for a, b in zip(res_batch, res_seq):
        assert (a["status"], a["rows"]) == (b["status"], b["rows"]) and a["nis"] == b["nis"] and np.array_equal(a["y"], b["y"])
    _results_match(res_batch, rr, "batch8")
    assert [r["status"] for r in res_batch] == [0, 0, 1, 0, 0, 0, 0, 0]
    _within(*batch, xr, Pr, TOL_STATE, "batch8")
    _invariants(*batch, "batch8")


def test_order_with_predictions(capi, oracle):
    table = {c["name"]: c for c in ac.cases()}
    c = table["position-rot0.3"]
    o1, o2 = c["obs"][0], table["wheel"]["obs"][0]
    rng = np.random.default_rng(11)
    steps = [(0.005 if i != 3 else 0.011, np.array([0.3, -0.1, 9.81]) + rng.normal(scale=0.2, size=3),
              np.array([0.02, -0.01, 0.3]) + rng.normal(scale=0.05, size=3)) for i in range(5)]
    x, P = c["x"].copy(), c["P"].copy()
    for i, (dt, a, g) in enumerate(steps):
        x, P = oracle.predict(x, P, dt, _Q(), a, g)
        if i == 2:
            x, P, r1 = ar.observe_one(oracle, x, P, o1)
    x, P, r2 = ar.observe_one(oracle, x, P, o2)
    assert r1["status"] == 0 and r2["status"] == 0
    got = {}
    for batch in (1, 0):
        with capi.Context() as ctx:
            ctx.set_option("batch_predict", batch)
            ctx.filter_set(c["x"], c["P"])
            for i, (dt, a, g) in enumerate(steps):
                ctx.predict(dt, _Q(), a, g)
                if i == 2:
                    ctx.observe([_rec(capi, o1)])
            ctx.observe([_rec(capi, o2)])
            got[batch] = ctx.filter_get()
    _within(*got[1], x, P, TOL_STATE, "3 predict, observe, 2 predict, observe")
    assert _same(got[1], got[0])
    # the order matters: the observation before the third prediction is another filter
    with capi.Context() as ctx:
        ctx.filter_set(c["x"], c["P"])
        for i, (dt, a, g) in enumerate(steps):
            if i == 2:
                ctx.observe([_rec(capi, o1)])
            ctx.predict(dt, _Q(), a, g)
        ctx.observe([_rec(capi, o2)])
        other = ctx.filter_get()
    assert np.abs(other[0] - got[1][0]).max() > 1e-6


def test_every_place_the_filter_can_be(capi, scene_small):
    sc = scene_small
    c = next(c for c in ac.cases() if c["name"] == "position-rot0.3")
    x0 = sc["x_init"]
    o = ac.obs(ac.POSITION, x0, 77, lever=ac.LEVER, innov=(0.02, -0.01, 0.015), gate=ac.CHI2_3_99)
    rec = _rec(capi, o)

    def fresh(state):   # what the observation makes of `state` in a context of its own, straight after lv_filter_set
        with capi.Context() as f:
            f.filter_set(*state)
            f.observe([rec])
            out = f.filter_get()
            assert f.observe_results()[0]["status"] == 0
            return out

    with capi.Context() as ctx, capi.Context() as twin:
        for k in (ctx, twin):
            k.map_build(sc["map_xyz"])
            k.scan_set(sc["scan_xyz"][:1500])
            k.filter_set(x0, sc["P0"])
            k.correct(want_passes=False)
        post = twin.filter_get()                     # (the posterior, from the twin: ctx's stays in kf and the mailbox)
        ctx.observe([rec])
        from_kf = ctx.filter_get()
        assert _same(from_kf, fresh(post)) and not _same(from_kf, post)
        # after lv_correct + lv_filter_get (the mailbox was read; the filter is still kf's)
        ctx.filter_set(x0, sc["P0"])
        ctx.correct(want_passes=False)
        assert _same(ctx.filter_get(), post)
        ctx.observe([rec])
        assert _same(ctx.filter_get(), from_kf)
        # the posterior copied to the filter's own buffer (mail_filter 0: lv_filter_get materialises), the mailbox still holding it
        ctx.set_option("mail_filter", 0)
        ctx.filter_set(x0, sc["P0"])
        ctx.correct(want_passes=False)
        assert _same(ctx.filter_get(), post)
        ctx.set_option("mail_filter", 1)
        ctx.observe([rec])
        assert _same(ctx.filter_get(), from_kf)
        # straight after lv_filter_set, and twice in a row
        ctx.filter_set(c["x"], c["P"])
        ctx.observe([_rec(capi, c["obs"][0])])
        once = ctx.filter_get()
        ctx.observe([rec])
        twice = ctx.filter_get()
    with capi.Context() as f:
        f.filter_set(c["x"], c["P"])
        f.observe([_rec(capi, c["obs"][0])])
        assert _same(f.filter_get(), once)
        f.filter_set(*once)
        f.observe([rec])
        assert _same(f.filter_get(), twice)


def test_feeding_the_lidar_update(capi, oracle, scene_small):
    sc = scene_small
    acc, gyro = np.array([0.05, -0.02, 9.809]), np.array([0.001, -0.002, 0.001])
    x0 = sc["x_init"]
    o = ac.obs(ac.POSITION, x0, 78, innov=sc["x_true"][:3] - x0[:3])   # a fix at the true position
    o["R"] = np.eye(3) * 1e-4
    rec = _rec(capi, o)
    with capi.Context() as ctx, capi.Context() as ref:
        for k in (ctx, ref):
            k.map_build(sc["map_xyz"])
            k.scan_set(sc["scan_xyz"])
            k.filter_set(x0, sc["P0"])
            k.predict(0.002, _Q(), acc, gyro)
            k.observe([rec])
        ctx.correct(want_passes=False)
        got = ctx.filter_get()
        mid = ref.filter_get()                       # the filter after the observation ...
        assert ref.observe_results()[0]["status"] == 0 and np.abs(mid[0][:3] - x0[:3]).max() > 1e-4
        ref.filter_set(*mid)                         # ... set by value: lv_correct's host-prior route
        ref.correct(want_passes=False)
        assert _same(got, ref.filter_get())
    # lv_map_add_scan after an observation transforms the scan with the observed state
    scan = sc["scan_xyz"][:700]
    shift = ac.obs(ac.POSITION, sc["x_true"], 79, innov=(0.5, -0.25, 0.125))
    with capi.Context() as ctx:
        ctx.filter_set(sc["x_true"], sc["P0"])
        ctx.scan_set(scan)
        ctx.observe([_rec(capi, shift)])
        ctx.map_add_scan(downsample=False)
        x_obs, _ = ctx.filter_get()
        got_map = ctx.map_fetch()
    assert np.abs(x_obs[:3] - sc["x_true"][:3]).max() > 1e-3
    want = oracle.transform_scan(x_obs, scan)
    assert np.array_equal(got_map.view(np.uint32), want.view(np.uint32))
    assert not np.array_equal(got_map, oracle.transform_scan(sc["x_true"], scan))


def test_arguments(capi):
    c = next(c for c in ac.cases() if c["name"] == "position-rot0.3")
    good = c["obs"][0]

    def spoiled(**kw):
        return _rec(capi, dict(good, **kw))

    nan, inf = float("nan"), float("inf")
    att = ac.obs(ac.ATTITUDE, c["x"], 5)
    bad = [spoiled(kind=0), spoiled(kind=5), spoiled(mask=0), spoiled(mask=8), spoiled(z=[nan, 0, 0, 0]), spoiled(z=[0, inf, 0, 0]),
           spoiled(R=np.full((3, 3), nan)), spoiled(lever=[0, nan, 0]), spoiled(gate=-1.0), spoiled(gate=nan),
           spoiled(kind=ac.VELOCITY_WORLD), spoiled(kind=ac.VELOCITY_BODY),          # (a lever arm with a kind that takes none)
           _rec(capi, dict(att, z=att["z"] * 1.001)), _rec(capi, dict(att, z=np.zeros(4)))]
    ok = _rec(capi, good)
    with capi.Context() as ctx:
        with pytest.raises(capi.LvError, match=r"error -4: lv_observe before lv_filter_set"):
            ctx.observe([ok])
        with pytest.raises(capi.LvError, match=r"error -4: lv_observe_results before lv_observe"):
            ctx.observe_results()
        ctx.filter_set(c["x"], c["P"])
        for k, b in enumerate(bad):
            with pytest.raises(capi.LvError, match=r"error -1: lv_observe: observation 1"):
                ctx.observe([ok, b, ok])
            with pytest.raises(capi.LvError, match=r"error -1: lv_observe: observation 0"):
                ctx.observe([b], wait=True)
        for n in (0, 9):
            with pytest.raises(capi.LvError, match=rf"error -1: lv_observe: {n} observations"):
                ctx.observe([ok] * n)
        assert capi.load_library().lv_observe(ctx.h, None, 1, None) == -1
        with pytest.raises(capi.LvError, match=r"error -4: lv_observe_results before lv_observe"):
            ctx.observe_results()                    # nothing was enqueued
        assert _same(ctx.filter_get(), (c["x"], c["P"]))
        # ... nor with a prediction waiting in the queue: it stays there, and the filter is the predicted one, not an observed one
        ctx.predict(0.01, _Q(), [0.1, 0.0, 9.8], [0.0, 0.01, 0.0])
        with pytest.raises(capi.LvError):
            ctx.observe([bad[0]])
        predicted = ctx.filter_get()
    with capi.Context() as ctx:
        ctx.filter_set(c["x"], c["P"])
        ctx.predict(0.01, _Q(), [0.1, 0.0, 9.8], [0.0, 0.01, 0.0])
        assert _same(ctx.filter_get(), predicted)
        # results: the capacity is judged, a short buffer writes nothing
        ctx.observe([ok, ok])
        out = (capi.ObserveResult * 1)()
        n = C.c_size_t(0)
        assert ctx.lib.lv_observe_results(ctx.h, out, 1, C.byref(n)) == -1 and n.value == 2
        assert len(ctx.observe_results()) == 2
