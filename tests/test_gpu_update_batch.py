"""lv_iterate_batch / lv_update_batch (limo-velo_amd/csrc/lv_batch.hip): every hypothesis of a batch is the single-pose call from
its own prior — passes and last-pass n_valid exactly, states to 1e-12 and covariances to 1e-9 relative against lv_update on both
routes (the batch runs the three-kernel route's search / fit / fold order, so it is expected to be bit-equal to that route) — and a
batch is independent of its neighbours, its order, its chunking and of everything the context keeps for single-pose calls."""
import math
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TOL_X, TOL_P_REL = 1e-12, 1e-9


@pytest.fixture(scope="module")
def capi(lv):
    from limo_velo_amd import capi as c

    return c


def _rot_yaw(x, deg):
    from limo_velo_amd import synth

    y = np.array(x, np.float64)
    y[3:7] = synth.quat_mul(synth.quat_from_rpy(0.0, 0.0, math.radians(deg)), y[3:7])
    return y


def _hypotheses(sc, m=37, seed=3):
    """x_init, x_true, perturbations up to 40 degrees of yaw and 3 m, one far outside the map; odd m."""
    rng = np.random.default_rng(seed)
    xs = [sc["x_init"], sc["x_true"]]
    far = np.array(sc["x_init"]); far[:3] += [5000.0, 5000.0, 0.0]
    xs.append(far)
    while len(xs) < m:
        x = _rot_yaw(sc["x_init"], rng.uniform(-40, 40) * rng.random() ** 2)
        x[:2] += rng.uniform(-3, 3, 2) * rng.random() ** 2
        xs.append(x)
    return np.array(xs)


def _singles(ctx, xs, P, fused):
    ctx.set_fused_pass(fused)
    out = [ctx.update(x, P) for x in xs]
    ctx.set_fused_pass(True)
    return out


def _agree(batch, singles, bit_exact=False, atol_x=TOL_X, atol_P=1e-13):
    bx, bP, bp, bl = batch
    for i, (x, P, n, _, sums) in enumerate(singles):
        assert bp[i] == n, (i, bp[i], n)
        assert bl[i]["n_valid"] == (sums[-1]["n_valid"] if n else 0), i
        if bit_exact:
            assert np.array_equal(bx[i], x), i
            assert bP is None or np.array_equal(bP[i], P), i
        else:
            np.testing.assert_allclose(bx[i], x, rtol=0, atol=atol_x)
            if bP is not None:
                np.testing.assert_allclose(bP[i], P, rtol=TOL_P_REL, atol=atol_P)
        if n:
            scale = max(1.0, np.abs(sums[-1]["HTH"]).max())
            assert np.abs(bl[i]["HTH"] - sums[-1]["HTH"]).max() <= 1e-12 * scale


def _same(a, b):
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2])
    assert (a[1] is None) == (b[1] is None) and (a[1] is None or np.array_equal(a[1], b[1]))
    for p, q in zip(a[3], b[3]):
        assert p["n_valid"] == q["n_valid"] and p["sum_h2"] == q["sum_h2"] and np.array_equal(p["HTH"], q["HTH"])


def test_each_hypothesis_is_lv_update(capi, oracle, scene_small):
    sc = scene_small
    xs = _hypotheses(sc)
    with capi.Context() as ctx:
        ctx.map_build(sc["map_xyz"])
        ctx.scan_set(sc["scan_xyz"])
        batch = ctx.update_batch(xs, sc["P0"], want_P=True)
        three = _singles(ctx, xs, sc["P0"], fused=False)
        fused = _singles(ctx, xs, sc["P0"], fused=True)
    _agree(batch, three, bit_exact=True)   # recorded: bit-equal to the three-kernel route
    _agree(batch, fused)
    p = batch[2]
    assert p[2] == 4 and batch[3][2]["n_valid"] == 0   # the hypothesis outside the map: every pass without matches
    assert p.min() < p.max()                            # some converge early
    tree = oracle.KdTree(sc["map_xyz"])
    for i in (0, 1, 5):
        xo, Po, po, _, so = oracle.update(xs[i], sc["P0"], sc["map_xyz"], sc["scan_xyz"], tree=tree)
        assert p[i] == po
        assert np.abs(batch[0][i] - xo).max() < 1e-9 and np.abs(batch[1][i] - Po).max() < 1e-9


def test_iterate_batch_is_lv_iterate(capi, scene_small):
    sc = scene_small
    xs = _hypotheses(sc, m=21)
    with capi.Context() as ctx:
        ctx.map_build(sc["map_xyz"])
        ctx.scan_set(sc["scan_xyz"])
        got = ctx.iterate_batch(xs)
        want = [ctx.iterate(x) for x in xs]
    for g, w in zip(got, want):
        assert g["n_valid"] == w["n_valid"]
        for k in ("HTH", "HTh", "sum_h2"):
            scale = max(1.0, np.abs(w[k]).max())
            assert np.abs(np.asarray(g[k]) - np.asarray(w[k])).max() <= 1e-12 * scale, k


def test_results_do_not_depend_on_the_batch(capi, scene_small):
    sc = scene_small
    xs = _hypotheses(sc)
    P = sc["P0"]
    with capi.Context() as ctx:
        ctx.map_build(sc["map_xyz"])
        ctx.scan_set(sc["scan_xyz"])
        ref = ctx.update_batch(xs, P, want_P=True)
        _same(ref, ctx.update_batch(xs, P, want_P=True))
        perm = np.random.default_rng(1).permutation(len(xs))
        b = ctx.update_batch(xs[perm], P, want_P=True)
        inv = np.argsort(perm)
        _same(ref, (b[0][inv], b[1][inv], b[2][inv], [b[3][i] for i in inv]))
        parts = [ctx.update_batch(xs[a:a + 10], P, want_P=True) for a in range(0, len(xs), 10)]
        _same(ref, (np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]), np.concatenate([p[2] for p in parts]),
                    sum((p[3] for p in parts), [])))
        one = ctx.update_batch(xs[4:5], P, want_P=True)
        _same((ref[0][4:5], ref[1][4:5], ref[2][4:5], ref[3][4:5]), one)
        dup = ctx.update_batch(np.concatenate([xs, xs[:5]]), P, want_P=True)
        _same(ref, (dup[0][:len(xs)], dup[1][:len(xs)], dup[2][:len(xs)], dup[3][:len(xs)]))
        _same((ref[0][:5], ref[1][:5], ref[2][:5], ref[3][:5]), (dup[0][len(xs):], dup[1][len(xs):], dup[2][len(xs):], dup[3][len(xs):]))
        ctx.set_option("batch_chunk_hypotheses", 4)
        _same(ref, ctx.update_batch(xs, P, want_P=True))


@pytest.mark.parametrize("kw,ext", [(dict(NUM_MATCH_POINTS=3), None), (dict(NUM_MATCH_POINTS=8), None), (dict(estimate_extrinsics=1), "xaloc"),
                                    (dict(degeneracy_mode=2), None), (dict(MAX_NUM_ITERS=0), None), (dict(MAX_NUM_ITERS=5), None),
                                    (dict(LiDAR_noise=1.0), None), (dict(LiDAR_noise=1e-6), None), (dict(LIMITS=[1.0] * 22 + [1e-12]), None),
                                    (dict(LIMITS=[1.0] * 23), None)])
def test_parameters(capi, scene_small, kw, ext):
    from limo_velo_amd import synth

    sc = synth.make_scene(50_000, 2_000, extrinsics=ext) if ext else scene_small
    xs = _hypotheses(sc, m=9)
    with capi.Context(capi.default_params(**kw)) as ctx:
        ctx.map_build(sc["map_xyz"])
        ctx.scan_set(sc["scan_xyz"])
        batch = ctx.update_batch(xs, sc["P0"], want_P=True)
        three = _singles(ctx, xs, sc["P0"], fused=False)
        fused = _singles(ctx, xs, sc["P0"], fused=True)
        _agree(batch, three, bit_exact=True)
        if ext:
            # the two single-pose routes themselves differ on hypotheses tens of degrees off once the extrinsics are estimated (up to
            # ~1e-11 in the weakly observed extrinsic rotation, ~2e-13 in the smallest covariance entries): the batch is held to the
            # three-kernel route bit for bit above and to the one-launch route within what separates the routes
            _agree(batch, fused, atol_x=1e-10, atol_P=1e-12)
        else:
            _agree(batch, fused)


def test_edges(capi, scene_small):
    sc = scene_small
    xs = _hypotheses(sc, m=5)
    with capi.Context() as ctx:
        lib = ctx.lib
        assert lib.lv_update_batch(ctx.h, None, 0, None, None, None, None) == 0
        assert lib.lv_iterate_batch(ctx.h, None, 0, None) == 0
        assert lib.lv_update_batch(ctx.h, None, 2, None, None, None, None) == -1
        assert lib.lv_iterate_batch(ctx.h, None, 2, None) == -1
        ctx.scan_set(sc["scan_xyz"])
        b = ctx.update_batch(xs, sc["P0"], want_P=True)                 # no map
        assert np.array_equal(b[0], xs) and not b[2].any() and all(d["n_valid"] == 0 for d in b[3])
        assert np.array_equal(b[1], np.broadcast_to(sc["P0"], b[1].shape))
        ctx.map_build(sc["map_xyz"])
        ctx.scan_set(np.zeros((0, 3), np.float32))                       # empty scan
        b = ctx.update_batch(xs, sc["P0"])
        assert np.array_equal(b[0], xs) and not b[2].any()
        assert all(d["n_valid"] == 0 for d in ctx.iterate_batch(xs))
        ctx.scan_set(sc["scan_xyz"])
        bad = xs.copy()
        bad[2, 0] = np.nan
        bad[3, 4] = np.inf
        b = ctx.update_batch(bad, sc["P0"], want_P=True)
        good = ctx.update_batch(xs[[0, 1, 4]], sc["P0"], want_P=True)
        _same((b[0][[0, 1, 4]], b[1][[0, 1, 4]], b[2][[0, 1, 4]], [b[3][i] for i in (0, 1, 4)]), good)
        for i in (2, 3):
            x, P, n, _, sums = ctx.update(bad[i], sc["P0"])
            assert b[2][i] == n and b[3][i]["n_valid"] == (sums[-1]["n_valid"] if n else 0)
            assert np.array_equal(np.isnan(b[0][i]), np.isnan(x))
            assert np.array_equal(b[0][i][~np.isnan(x)], x[~np.isnan(x)])


def test_the_batch_leaves_the_context_alone(capi, scene_small):
    sc = scene_small
    xs = _hypotheses(sc, m=7)
    Q = np.eye(12) * 1e-4
    acc, gyro = np.array([0.0, 0.0, 9.81]), np.zeros(3)
    out = []
    for with_batch in (False, True):
        with capi.Context() as ctx:
            ctx.map_build(sc["map_xyz"])
            ctx.scan_set(sc["scan_xyz"])
            ctx.filter_set(sc["x_init"], sc["P0"])
            for _ in range(3):
                ctx.predict(0.01, Q, acc, gyro)
            if with_batch:
                ctx.update_batch(xs, sc["P0"])
            ctx.correct()
            out.append(ctx.filter_get())
            passes = ctx.last_passes()
            ctx.update_batch(xs, sc["P0"])
            assert ctx.last_passes() == passes
            ctx.iterate(sc["x_init"])
            knn, matches = ctx.fetch_knn(), ctx.fetch_matches()
            lp = ctx.last_passes()
            ctx.iterate_batch(xs)
            ctx.update_batch(xs, sc["P0"])
            for a, b in zip(knn, ctx.fetch_knn()):
                assert np.array_equal(a, b)
            for a, b in zip(matches, ctx.fetch_matches()):
                assert np.array_equal(a, b)
            assert ctx.last_passes() == lp
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])


def test_map_state(capi, scene_small):
    sc = scene_small
    xs = _hypotheses(sc, m=9)
    P = sc["P0"]
    m = sc["map_xyz"]
    with capi.Context() as ctx, capi.Context() as ref:
        ctx.scan_set(sc["scan_xyz"])
        ref.scan_set(sc["scan_xyz"])
        ctx.map_build(m[:30_000])
        ctx.map_add(m[30_000:])                       # no sync: the batch is ordered behind the insert
        ref.map_build(m)
        _same(ref.update_batch(xs, P, want_P=True), ctx.update_batch(xs, P, want_P=True))
        n = ctx.map_evict_box([-5.0, -5.0, -50.0], [5.0, 5.0, 50.0], keep_inside=False)
        assert n > 0
        ref.map_build(ctx.map_fetch())
        after_evict = ctx.update_batch(xs, P, want_P=True)
        _same(ref.update_batch(xs, P, want_P=True), after_evict)
        ctx.map_relinearise_async()
        during = ctx.update_batch(xs, P, want_P=True)
        ctx.map_rebuild_status(wait=True)
        _same(during, ctx.update_batch(xs, P, want_P=True))
        _same(during, after_evict)


def test_prior_map_round_trip(capi, scene_small, tmp_path):
    from limo_velo_amd import prelocalise as pl

    sc = scene_small
    xs = _hypotheses(sc, m=11)
    m = sc["map_xyz"]
    path = os.path.join(tmp_path, "map.npy")
    with capi.Context() as ctx:
        ctx.map_build(m[:20_000])
        ctx.map_add(m[20_000:35_000])
        ctx.map_add(m[35_000:])
        ctx.map_evict_box([0.0, 0.0, -50.0], [6.0, 6.0, 50.0], keep_inside=False)
        ctx.scan_set(sc["scan_xyz"])
        a = ctx.update_batch(xs, sc["P0"], want_P=True)
        pl.save_map(ctx, path)
    with capi.Context() as ctx:
        pl.load_map(ctx, path)
        ctx.scan_set(sc["scan_xyz"])
        _same(a, ctx.update_batch(xs, sc["P0"], want_P=True))


def test_prelocalisation_end_to_end(capi, scene_small):
    """Grid: yaw +-45 deg in 7.5 deg steps, xy +-1.5 m in 0.5 m steps (13 x 49 = 637 hypotheses) around a prior 1 m and 25 deg off;
    keep 8, rounds = 3."""
    from limo_velo_amd import prelocalise as pl

    sc = scene_small
    prior = _rot_yaw(sc["x_true"], 25.0)
    prior[:2] += [0.8, -0.6]
    grid = dict(xy_radius=1.5, xy_step=0.5, yaw_span=math.radians(45), yaw_step=math.radians(7.5))
    with capi.Context() as ctx:
        ctx.map_build(sc["map_xyz"])
        ctx.scan_set(sc["scan_xyz"])
        cand = pl.candidate_grid(prior, **grid)
        assert len(cand) == 637
        raw = ctx.iterate_batch(cand)   # the grid points themselves, ranked by their own measurement pass
        top = cand[pl.rank(np.zeros(len(cand), np.int32), raw)[0]]
        best, table = pl.prelocalise(ctx, prior, sc["P0"], rounds=3, keep=8, **grid)
    d_xy = np.linalg.norm(top[:2] - sc["x_true"][:2])
    q = top[3:7]
    qt = sc["x_true"][3:7]
    d_yaw = math.degrees(2 * math.acos(min(1.0, abs(float(np.dot(q, qt))))))
    # the top raw grid point has the grid's nearest yaw (2.5 degrees off); the match count of an unrefined pose does not single
    # out the nearest xy (measured: 1.43 m off), which is why the grid is refined before it is ranked
    assert d_yaw <= 3.75, (d_xy, d_yaw)
    assert np.linalg.norm(best[:3] - sc["x_true"][:3]) < 5e-3
    ang = math.degrees(2 * math.acos(min(1.0, abs(float(np.dot(best[3:7], qt))))))
    assert ang < 0.1, ang
    assert table[0]["n_valid"] > 0


def test_scale(capi):
    from limo_velo_amd import synth

    sc = synth.make_scene(1_000_000, 8_192)
    rng = np.random.default_rng(7)
    for m, n in ((512, 2048), (4096, 8192)):
        xs = np.repeat(sc["x_init"][None], m, 0)
        for i in range(m):
            xs[i] = _rot_yaw(xs[i], rng.uniform(-20, 20))
            xs[i, :2] += rng.uniform(-1.5, 1.5, 2)
        with capi.Context() as ctx:
            ctx.map_build(sc["map_xyz"])
            ctx.scan_set(sc["scan_xyz"][:n])
            # (m = 4096, n = 8192: 4 GiB of hand-over records against a 256 MiB budget, so 16 chunks of 256 hypotheses)
            batch = ctx.update_batch(xs, sc["P0"], want_P=True)
            pick = rng.choice(m, 16, replace=False)
            singles = _singles(ctx, xs[pick], sc["P0"], fused=False)
            _agree((batch[0][pick], batch[1][pick], batch[2][pick], [batch[3][i] for i in pick]), singles)
