"""GPU tests of lv_map_remove_dynamic (lv_visibility.hip): free-space removal of dynamic points against the numpy statement of
the rule in tests/visibility_ref.py.  Counts must equal the reference on every point whose count the f32 arithmetic cannot change
(see there); the share of the others is reported and bounded.  Views are ray-cast sweeps whose rays go through pixel centres
(synth.ring_sweep), or random returns kept off bin edges (visibility_ref.edge_safe)."""
import ctypes as C
import math
import time

import numpy as np
import pytest

import visibility_ref as vr

pytestmark = pytest.mark.gpu

LV_EINVAL = -1


@pytest.fixture(scope="module")
def capi(lv):
    from limo_velo_amd import capi as c

    return c


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _moved(x0, dx, dy, dyaw):
    from limo_velo_amd import synth

    x = np.array(x0, np.float64)
    x[0] += dx
    x[1] += dy
    x[3:7] = synth.quat_mul(x[3:7], synth.quat_from_rpy(0.0, 0.0, math.radians(dyaw)))
    return x


def _ghost_box(c, size, z0, z1, n, seed):
    """n points on the four sides and the top of an axis-aligned box (a parked car, a pedestrian): no bottom, it stands on the ground."""
    rng = np.random.default_rng(seed)
    u = rng.uniform(size=(n, 3))
    f = rng.integers(0, 5, n)
    x0, y0 = c[0] - size[0] / 2, c[1] - size[1] / 2
    p = np.empty((n, 3))
    p[:, 0] = np.where(f == 0, x0, np.where(f == 1, x0 + size[0], x0 + u[:, 0] * size[0]))
    p[:, 1] = np.where(f == 2, y0, np.where(f == 3, y0 + size[1], y0 + u[:, 1] * size[1]))
    p[:, 2] = np.where(f == 4, z1, z0 + u[:, 2] * (z1 - z0))
    return p.astype(np.float32)


def _ghosts():
    return np.concatenate([_ghost_box((-2.5, 7.53), (2.0, 1.2), 0.4, 1.5, 2000, 1), _ghost_box((-2.5, -11.5), (0.8, 0.8), 0.3, 1.4, 1000, 2)])


def _views(capi, synth, rects, states, rings=64, az=2048, fov=(-25.0, 3.0), seed=11):
    out = []
    for i, s in enumerate(states):
        R, t = capi.sensor_pose(s)
        out.append((R, t, synth.ring_sweep(rects, R, t, rings, az, fov, range_sigma=0.01, seed=seed + i)))
    return out


@pytest.fixture(scope="module")
def scene(capi):
    from limo_velo_amd import synth

    M = 200_000
    sc = synth.make_ring_scene(M, 16, 512)
    rects = synth.scene_surfaces(M)
    x0 = sc["x_true"]
    states = [x0, _moved(x0, 4.0, 1.0, 20.0), _moved(x0, -2.0, 3.5, -15.0)]
    return dict(sc=sc, rects=rects, states=states, views=_views(capi, synth, rects, states))


def _check(hits, lo, hi, judged, what):
    hits = np.asarray(hits, np.int64)
    exact = lo == hi
    bad = np.flatnonzero(exact & (hits != lo))
    assert bad.size == 0, f"{what}: {bad.size} counts differ from the reference, first {bad[:8]} got {hits[bad[:8]]} want {lo[bad[:8]]}"
    assert np.all((hits >= lo) & (hits <= hi)), f"{what}: a count outside its admissible interval"
    share = float((~exact).sum()) / max(int(judged.sum()), 1)
    print(f"{what}: {int(judged.sum())} judged, {int((~exact).sum())} ambiguous ({100 * share:.3f} %), {int((hits > 0).sum())} seen through")
    assert share < 0.005, share
    return ~exact


@pytest.mark.parametrize("n_views", [1, 3, 32])
def test_classification_matches_the_reference_and_leaves_the_map(capi, scene, n_views):
    from limo_velo_amd import synth

    sc = scene["sc"]
    mp = np.concatenate([sc["map_xyz"], _ghosts()])
    if n_views == 32:   # 32 poses around the first one, 32 x 1024 sweeps, a wider window
        rng = np.random.default_rng(5)
        states = [_moved(scene["states"][0], *rng.uniform(-5, 5, 2), rng.uniform(-180, 180)) for _ in range(32)]
        views = _views(capi, synth, scene["rects"], states, rings=32, az=1024, seed=100)
        prm = capi.default_visibility_params(width=1024, height=32, window=2, min_hits=3)
    else:
        views = scene["views"][:n_views]
        prm = capi.default_visibility_params()
    with capi.Context() as ctx:
        ctx.map_build(mp)
        before, stats = ctx.map_fetch(), ctx.map_stats()
        n, hits = ctx.map_remove_dynamic(views, prm, dry_run=True)
        assert n == 0 and len(hits) == len(mp)
        assert np.array_equal(_bits(ctx.map_fetch()), _bits(before)) and ctx.map_stats() == stats
    lo, hi, judged = vr.hits(mp, views, prm)
    _check(hits, lo, hi, judged, f"{n_views} views")
    assert (hits > 0).sum() > 100


def test_wrap_fov_range_empty_windows_non_finite_and_empty_views(capi):
    """A synthetic scene around one sensor: returns at 30 m only in the columns next to +-pi (seen through the wrap by the window),
    random returns elsewhere, NaN / inf returns, a view without returns; map points inside and outside the rows and the ranges."""
    rng = np.random.default_rng(3)
    prm = capi.default_visibility_params(width=256, height=16, window=2, min_range=1.0, max_range=40.0)
    W, H = prm.width, prm.height
    inv_col, v_min, inv_row = vr.geometry(prm)

    def at(col, row, r):   # sensor-frame points at pixel coordinates (col, row) and ranges r
        az = col / inv_col - math.pi
        el = v_min + row / inv_row
        return np.stack([r * np.cos(el) * np.cos(az), r * np.cos(el) * np.sin(az), r * np.sin(el)], axis=1).astype(np.float32)

    n = 4000
    wrap_ret = at(np.where(rng.uniform(size=n) < 0.5, 0.5, W - 0.5), rng.integers(0, H, n) + 0.5, np.full(n, 30.0))
    other = at(rng.uniform(40, W - 40, n), rng.uniform(0, H, n), rng.uniform(0.5, 60, n))
    bad = np.array([[np.nan, 1, 1], [np.inf, 0, 0], [1, -np.inf, 2], [0.5, 0.1, 0.0]], np.float32)
    ret = vr.edge_safe(np.concatenate([wrap_ret, other, bad]), prm)
    m = 30000
    mcol = np.concatenate([rng.uniform(-3, 3, m // 3) % W, rng.uniform(0, W, m - m // 3)])
    mrow = rng.uniform(-3, H + 3, m)                 # some outside the rows
    mr = rng.uniform(0.2, 50, m)                     # some outside [min_range, max_range]
    local = at(mcol, mrow, mr)
    R = np.asarray(capi.sensor_pose(np.r_[[5.0, -3.0, 1.2], 0.05, -0.02, 0.6, math.sqrt(1 - 0.05 ** 2 - 0.02 ** 2 - 0.6 ** 2),
                                          [0, 0, 0, 1], np.zeros(3), np.zeros(12)])[0], np.float32)
    t = np.array([5.0, -3.0, 1.2], np.float32)
    mp = (local.astype(np.float64) @ R.T.astype(np.float64) + t).astype(np.float32)
    views = [(R, t, ret), (R, t, np.zeros((0, 3), np.float32))]
    with capi.Context() as ctx:
        ctx.map_build(mp)
        before = ctx.map_fetch()
        _, hits = ctx.map_remove_dynamic(views, prm, dry_run=True)
        assert np.array_equal(_bits(ctx.map_fetch()), _bits(before))
    lo, hi, judged = vr.hits(mp, views, prm)
    _check(hits, lo, hi, judged, "synthetic")
    assert hits.max() <= 1   # the empty view gives no evidence
    near_wrap = ((mcol < 2.5) | (mcol > W - 2.5)) & (mrow >= 0.01) & (mrow < H - 0.01) & (mr > 1.01) & (mr < 29)
    assert hits[near_wrap & (lo == hi)].min() == 1 and near_wrap.sum() > 100
    assert np.all(hits[(mr < 0.99) | (mr > 40.01) | (mrow < -0.01) | (mrow > H + 0.01)] == 0)


def _np_knn(map_xyz, q, k):
    """(idx, d2 bits): brute force in calc_dist's f32 order, sorted on (d2, index)."""
    m = np.asarray(map_xyz, np.float32)
    ar = np.arange(len(m), dtype=np.uint64)[None, :]
    keys = []
    for s in range(0, len(q), 16):
        d = np.asarray(q[s:s + 16], np.float32)[:, None, :] - m[None, :, :]
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        key = (d2.view(np.uint32).astype(np.uint64) << np.uint64(32)) | ar
        keys.append(np.sort(np.partition(key, k - 1, axis=1)[:, :k], axis=1))
    key = np.concatenate(keys)
    return (key & np.uint64(0xFFFFFFFF)).astype(np.uint32), (key >> np.uint64(32)).astype(np.uint32)


def test_removal_end_to_end(capi, scene):
    sc = scene["sc"]
    static = sc["map_xyz"]
    g = _ghosts()
    mp = np.concatenate([static, g])
    ns = len(static)
    prm = capi.default_visibility_params(min_hits=2)
    lo, hi, judged = vr.hits(mp, scene["views"], prm)
    with capi.Context() as ctx:
        ctx.map_build(mp)
        before = ctx.map_fetch()
        n, hits = ctx.map_remove_dynamic(scene["views"], prm)
        amb = _check(hits, lo, hi, judged, "removal")
        gone = hits >= 2
        assert n == int(gone.sum()) and ctx.map_size() == len(mp) - n
        after = ctx.map_fetch()
        assert np.array_equal(_bits(after), _bits(before[~gone]))
        assert np.all(gone[ns:][(lo[ns:] >= 2) & ~amb[ns:]]), "a ghost point the reference removes is still there"
        assert not gone[:ns].any(), f"{int(gone[:ns].sum())} static points removed"
        assert gone[ns:].mean() >= 0.9, gone[ns:].mean()
        L = float(sc["L"])
        wall_or_ground = (np.abs(static[:, 2]) < 0.05) | (np.abs(np.abs(static[:, 0]) - L) < 0.05) | (np.abs(np.abs(static[:, 1]) - L) < 0.05)
        assert not gone[:ns][wall_or_ground].any()
        print(f"removed {n}: {int(gone[ns:].sum())} of {len(g)} ghost points")
        q = after[np.random.default_rng(1).integers(0, len(after), 300)] + np.float32(0.05)
        idx, d2, _ = ctx.map_knn(q, 5)
        ri, rd = _np_knn(after, q, 5)
        assert np.array_equal(idx, ri) and np.array_equal(_bits(d2), rd)
        ctx.scan_set(sc["scan_xyz"])
        x1, P1, p1, _, _ = ctx.update(sc["x_init"], sc["P0"])
    with capi.Context() as fresh:
        fresh.map_build(after)
        fresh.scan_set(sc["scan_xyz"])
        x2, P2, p2, _, _ = fresh.update(sc["x_init"], sc["P0"])
    assert p1 == p2 and np.array_equal(x1.view(np.uint64), x2.view(np.uint64)) and np.array_equal(P1.view(np.uint64), P2.view(np.uint64))


def _raw_remove(capi, ctx, views, prm):
    keep = []
    arr = (capi.View * len(views))()
    for i, (R, t, pts) in enumerate(views):
        a = np.ascontiguousarray(pts, np.float32)
        keep.append(a)
        arr[i].R[:] = [float(v) for v in np.asarray(R, np.float32).ravel()]
        arr[i].t[:] = [float(v) for v in np.asarray(t, np.float32).ravel()]
        arr[i].points, arr[i].stride, arr[i].n = a.ctypes.data, 12, len(a)
    nr = C.c_size_t(0)
    rc = ctx.lib.lv_map_remove_dynamic(ctx.h, arr, C.c_size_t(len(views)), C.byref(prm), None, C.byref(nr))
    return rc, int(nr.value)


def test_removal_sees_a_pending_insert_and_interleaves_like_the_synchronous_sequence(capi, scene):
    sc = scene["sc"]
    prm = capi.default_visibility_params(min_hits=2)
    g = _ghosts()
    x0 = np.asarray(scene["states"][0])
    # the ghosts as a scan of the first pose, inserted by lv_map_add_scan with that state; the removal is issued right behind it
    R, t = capi.sensor_pose(x0)
    scan = ((g.astype(np.float64) - t.astype(np.float64)) @ R.astype(np.float64)).astype(np.float32)
    with capi.Context() as ctx:
        ctx.map_build(sc["map_xyz"])
        ctx.scan_set(scan)
        ctx.filter_set(x0, sc["P0"])
        ctx.map_add_scan(downsample=False)
        rc, n = _raw_remove(capi, ctx, scene["views"], prm)
        assert rc == 0
        after = ctx.map_fetch()
    with capi.Context() as ref:
        ref.map_build(sc["map_xyz"])
        ref.scan_set(scan)
        ref.filter_set(x0, sc["P0"])
        ref.map_add_scan(downsample=False)
        ref.synchronize()
        full = ref.map_fetch()
        _, hits = ref.map_remove_dynamic(scene["views"], prm, dry_run=True)
    assert len(full) > len(sc["map_xyz"]) and n == int((hits >= 2).sum()) and n > 0.9 * len(g)
    assert np.array_equal(_bits(after), _bits(full[hits < 2]))

    rng = np.random.default_rng(9)
    extra = [g[rng.permutation(len(g))[:1500]] + np.float32(0.01), (rng.uniform(-1, 1, (800, 3)) * [3, 3, 0.5] + [2, 12, 1]).astype(np.float32)]
    lo_b, hi_b = np.array([-30, -30, -1], np.float32), np.array([30, 30, 9], np.float32)

    def run(ctx, sync):
        steps = [lambda: ctx.map_add(g), lambda: ctx.map_remove_dynamic(scene["views"][:2], capi.default_visibility_params(min_hits=1)),
                 lambda: ctx.map_evict_box(lo_b, hi_b, keep_inside=True), lambda: ctx.map_add(extra[0]), lambda: ctx.map_add(extra[1]),
                 lambda: _raw_remove(capi, ctx, scene["views"], prm)]
        for s in steps:
            s()
            if sync:
                ctx.synchronize()
        return ctx.map_fetch()

    with capi.Context() as a, capi.Context() as b:
        a.map_build(sc["map_xyz"])
        b.map_build(sc["map_xyz"])
        assert np.array_equal(_bits(run(a, False)), _bits(run(b, True)))


def test_removal_during_a_background_rebuild(capi, scene):
    sc = scene["sc"]
    g = _ghosts()
    prm = capi.default_visibility_params(min_hits=2)

    def run(ctx, background):
        ctx.set_option("async_relinearise", 1 if background else 0)
        ctx.map_build(np.concatenate([sc["map_xyz"], g]))
        ctx.map_evict_box(np.array([-1e3, -1e3, -1e3], np.float32), np.array([1e3, 0.0, 1e3], np.float32), keep_inside=False)
        journaled = 0
        if background:
            ctx.set_option("async_relinearise_test_delay_ms", 400)
            ctx.map_relinearise_async()
            t0 = time.monotonic()
            while ctx.map_rebuild_status()["state"] in (4, 5) and time.monotonic() - t0 < 10:   # until the snapshot is taken
                ctx.map_size()
                time.sleep(0.001)
            assert ctx.map_rebuild_status()["state"] == 1
        ctx.map_add(g[:500] + np.float32(0.02))
        ctx.map_remove_dynamic(scene["views"], prm)
        journaled = max(journaled, ctx.map_rebuild_status()["journal"])
        ctx.map_add(g[500:] - np.float32(0.02))
        ctx.map_remove_dynamic(scene["views"][1:], capi.default_visibility_params(min_hits=1))
        journaled = max(journaled, ctx.map_rebuild_status()["journal"])
        st = ctx.map_rebuild_status(wait=True)
        return ctx.map_fetch(), st, journaled

    with capi.Context() as a:
        fa, sa, ja = run(a, True)
    with capi.Context() as b:
        fb, _, _ = run(b, False)
    assert sa["adopted"] >= 1 and sa["state"] == 0 and ja >= 1, (sa, ja)
    assert np.array_equal(_bits(fa), _bits(fb))


def test_invalid_arguments_change_nothing(capi, scene):
    sc = scene["sc"]
    v = scene["views"][0]
    bad = [dict(width=0), dict(height=0), dict(width=2048, height=513), dict(v_min_deg=3.0, v_max_deg=3.0), dict(v_min_deg=float("nan")),
           dict(min_range=0.0), dict(min_range=90.0), dict(max_range=float("inf")), dict(margin_abs=0.0), dict(margin_rel=-0.1),
           dict(margin_abs=float("nan")), dict(window=-1), dict(window=9), dict(min_hits=0), dict(min_hits=2)]
    with capi.Context() as ctx:
        ctx.map_build(sc["map_xyz"])
        before, stats = ctx.map_fetch(), ctx.map_stats()
        for kw in bad:
            rc, n = _raw_remove(capi, ctx, [v], capi.default_visibility_params(**kw))
            assert rc == LV_EINVAL and n == 0, kw
        prm = capi.default_visibility_params()
        for views in ([], [v] * 33):
            arr = (capi.View * max(len(views), 1))()
            assert ctx.lib.lv_map_remove_dynamic(ctx.h, arr, C.c_size_t(len(views)), C.byref(prm), None, None) == LV_EINVAL
        nan_pose = (np.full((3, 3), np.nan, np.float32), v[1], v[2])
        assert _raw_remove(capi, ctx, [nan_pose], prm)[0] == LV_EINVAL
        arr = (capi.View * 1)()
        arr[0].n, arr[0].stride = 10, 12   # points NULL
        assert ctx.lib.lv_map_remove_dynamic(ctx.h, arr, C.c_size_t(1), C.byref(prm), None, None) == LV_EINVAL
        assert ctx.lib.lv_map_remove_dynamic(ctx.h, None, C.c_size_t(1), C.byref(prm), None, None) == LV_EINVAL
        assert np.array_equal(_bits(ctx.map_fetch()), _bits(before)) and ctx.map_stats() == stats
    with capi.Context() as empty:   # an empty map: LV_OK, nothing removed
        assert _raw_remove(capi, empty, [v], capi.default_visibility_params()) == (0, 0)


def test_scale_one_million_points_eight_views(capi):
    from limo_velo_amd import synth

    M = 1_000_000
    sc = synth.make_ring_scene(M, 16, 512)
    rects = synth.scene_surfaces(M)
    rng = np.random.default_rng(8)
    states = [_moved(sc["x_true"], *rng.uniform(-8, 8, 2), rng.uniform(-180, 180)) for _ in range(8)]
    views = _views(capi, synth, rects, states, seed=200)
    mp = np.concatenate([sc["map_xyz"], _ghosts()])
    prm = capi.default_visibility_params(min_hits=3)
    with capi.Context() as ctx:
        ctx.map_build(mp)
        n, hits = ctx.map_remove_dynamic(views, prm, dry_run=True)
    lo, hi, judged = vr.hits(mp, views, prm)
    _check(hits, lo, hi, judged, "1 M points, 8 views")
