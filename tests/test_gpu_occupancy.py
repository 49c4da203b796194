"""GPU tests of the occupancy grid (lv_occupancy.hip; include/limovelo_hip.h "Occupancy grid") against the numpy statement of the
rule in tests/occupancy_ref.py.  The rule is integer arithmetic after one quantisation step, so everything is held to equality:
log-odds as bits (NaN by isnan), stats as integers, no tolerance anywhere."""
import ctypes as C
import math

import numpy as np
import pytest

import occupancy_ref as ocr

pytestmark = pytest.mark.gpu

LV_EINVAL, LV_ESTATE = -1, -4
F = np.float32
ID = np.eye(3, dtype=F)


@pytest.fixture(scope="module")
def capi(lv):
    from limo_velo_amd import capi as c

    return c


def _cparams(capi, prm):
    return capi.default_occupancy_params(**prm)


def _moved(x0, dx, dy, dyaw):
    from limo_velo_amd import synth

    x = np.array(x0, np.float64)
    x[0] += dx
    x[1] += dy
    x[3:7] = synth.quat_mul(x[3:7], synth.quat_from_rpy(0.0, 0.0, math.radians(dyaw)))
    return x


# The room of the 20k-point scene is the square |x|, |y| <= 6.18 m with walls 8 m high.  The grid starts at x = -1.75 and
# z = -0.75: the third pose (x = -4) stands outside it, every sweep's returns on the wall x = -6.18 end outside it, and with
# max_range 8 m the long rays are cut.
SCENE_PRM = ocr.params(origin=(-1.75, -9.25, -0.75), resolution=0.5, nx=96, ny=80, nz=24, min_range=1.0, max_range=8.0)


@pytest.fixture(scope="module")
def scene(capi):
    """The three sweeps and the reference after each of them (computed once, never written to)."""
    from limo_velo_amd import synth

    M = 20_000
    sc = synth.make_ring_scene(M, 16, 256)
    rects = synth.scene_surfaces(M)
    x0 = sc["x_true"]
    views = []
    for i, s in enumerate([x0, _moved(x0, 2.0, 1.0, 20.0), _moved(x0, -7.0, 3.5, -15.0)]):
        R, t = capi.sensor_pose(s)
        views.append((R, t, synth.ring_sweep(rects, R, t, 16, 256, range_sigma=0.01, seed=11 + i)))
    prm = SCENE_PRM
    after, stats = [], []
    L = ocr.empty(prm)
    for v in views:
        L, st = ocr.integrate(prm, L, [v])
        after.append(L)
        stats.append(st)
    # what the placement is for
    assert ocr.view_origin(prm, views[2][1])[0] < 0 <= ocr.view_origin(prm, views[0][1])[0]
    for R, t, pts in views:
        v = ocr.returns(prm, R, t, pts)[0] >> 8
        inside = np.all((v >= 0) & (v < np.array([prm["nx"], prm["ny"], prm["nz"]])), axis=1)
        assert inside.any() and (~inside).any()
    assert all(int(s[1]) > 0 for s in stats)   # (cut rays in every sweep)
    for a in after:
        a.setflags(write=False)
    return dict(sc=sc, views=views, prm=prm, after=after, stats=stats)


def _run_scene(capi, scene):
    out = []
    with capi.Context() as ctx:
        ctx.occ_configure(_cparams(capi, scene["prm"]))
        for v in scene["views"]:
            st = ctx.occ_integrate([v])
            out.append((ctx.occ_fetch(), st))
    return out


def _hold(capi, prm, views, one_call=True):
    """The GPU's grid and stats after views equal the reference's; returns the grid."""
    ref, rstats = ocr.integrate(prm, ocr.empty(prm), views)
    with capi.Context() as ctx:
        ctx.occ_configure(_cparams(capi, prm))
        if one_call:
            stats = ctx.occ_integrate(views)
        else:
            stats = sum((ctx.occ_integrate([v]) for v in views), np.zeros(4, np.uint64))
        L = ctx.occ_fetch()
    assert ocr.same_bits(L, ref), f"{np.sum(~((L == ref) | (np.isnan(L) & np.isnan(ref))))} voxels differ"
    assert list(stats) == list(rstats)
    return L


# ---- 1. sweeps in a scene
def test_sweeps_in_a_scene(capi, scene):
    for (L, st), ref, rst in zip(_run_scene(capi, scene), scene["after"], scene["stats"]):
        assert ocr.same_bits(L, ref), f"{np.sum(~((L == ref) | (np.isnan(L) & np.isnan(ref))))} voxels differ"
        assert list(st) == list(rst)
    assert list(np.sum(scene["stats"], axis=0))[2] > 1000


# ---- 2. word tails and tiny grids
@pytest.mark.parametrize("dims", [(33, 5, 3), (31, 4, 2), (1, 6, 5), (1, 1, 1)])
def test_word_tails_and_tiny_grids(capi, dims):
    nx, ny, nz = dims
    rng = np.random.default_rng(nx)
    prm = ocr.params(origin=(0.0, 0.0, 0.0), resolution=0.5, nx=nx, ny=ny, nz=nz, min_range=0.05, max_range=10.0)
    hi = np.array(dims) * 0.5
    views = []
    for t in (hi * 0.5, hi + 0.7):   # the sensor inside the grid, and outside it
        ends = rng.uniform(-1.0, 1.0, (2000, 3)) * (hi + 2.0) + hi * 0.5
        views.append((ID, t.astype(F), (ends - t).astype(F)))
    _hold(capi, prm, views[:1])
    _hold(capi, prm, views[1:])
    _hold(capi, prm, views)


# ---- 3. degenerate rays
DEG_PRM = ocr.params(origin=(-2.0, -1.5, -1.0), resolution=0.25, nx=19, ny=13, nz=9, min_range=0.3, max_range=4.0)


def test_degenerate_rays(capi):
    t = np.array([0.125, 0.125, 0.125], F)   # the centre of voxel (8, 6, 4)
    ax = [(sgn * r * np.eye(3)[a]) for a in range(3) for sgn in (1, -1) for r in (0.5, 1.0, 3.0, 5.0)]
    diag = [np.array([sx, sy, sz]) * r for sx in (1, -1) for sy in (1, -1) for sz in (1, -1) for r in (0.25, 0.75, 1.0, 2.5)]
    plane = [np.array([r, -r, 0.0]) for r in (0.5, 1.5)] + [np.array([0.0, r, r]) for r in (0.5, 1.5)]
    rays = np.array(ax + diag + plane, F)
    _hold(capi, DEG_PRM, [(ID, t, rays)])
    _hold(capi, DEG_PRM, [(ID, np.zeros(3, F), rays)])                                     # from a lattice corner
    _hold(capi, DEG_PRM, [(ID, np.array([0.25, 0.1, 0.1], F), np.array([[-1.0, 0.01, 0.0], [-0.4, -0.4, -0.4]], F))])   # n = 0
    # a return in the sensor's own voxel (zero steps; hit wins over the free of the ray through it), non-finite returns, a return
    # below min_range, a cut return (its end voxel is free)
    prm = dict(DEG_PRM, resolution=1.0, origin=(-4.0, -4.0, -4.0), nx=8, ny=8, nz=8, max_range=3.0)
    pts = np.array([[0.3, 0.01, 0.0], [1.0, 0.0, 0.0], [np.nan, 0, 0], [0, -np.inf, 0], [0.05, 0, 0], [0.0, 30.0, 0.0]], F)
    L = _hold(capi, prm, [(ID, np.array([0.2, 0.2, 0.2], F), pts)])
    assert L[4, 4, 4] == F(0.85) and L[4, 4, 5] == F(0.85)
    assert list(L[4, 4:8, 4]) == [F(0.85)] + [F(-0.4)] * 3 and np.isnan(L).sum() == 8 ** 3 - 5
    # two rays of one view, one crossing the voxel the other hits: l_hit only
    L = _hold(capi, DEG_PRM, [(ID, t, np.array([[1.0, 0, 0], [2.0, 0, 0]], F))])
    assert L[4, 6, 12] == F(0.85) and L[4, 6, 16] == F(0.85) and L[4, 6, 11] == F(-0.4)
    # a view with n = 0, one with a non-finite t and one too far away give no evidence; the view between them does
    views = [(ID, t, np.zeros((0, 3), F)), (ID, np.array([np.nan, 0, 0], F), rays), (ID, t, rays), (ID, np.array([0, 3000.0, 0], F), rays)]
    L = _hold(capi, DEG_PRM, views)
    assert ocr.same_bits(L, ocr.integrate(DEG_PRM, ocr.empty(DEG_PRM), views[2:3])[0])


# ---- 4. order and clamping
def test_order_and_clamping(capi, scene):
    t = np.array([0.125, 0.125, 0.125], F)
    view = (ID, t, np.array([[1.0, 0, 0], [2.0, 0, 0], [0, -0.8, 0.3]], F))
    L = _hold(capi, DEG_PRM, [view] * 12)
    assert L[4, 6, 12] == F(3.5) and L[4, 6, 11] == F(-2.0)
    # 32 different views in one call = 32 calls of one view = the reference; the order shows (free, hit, free on shared voxels)
    rng = np.random.default_rng(4)
    views = []
    for i in range(32):
        d = rng.normal(size=(60, 3))
        d /= np.linalg.norm(d, axis=1)[:, None]
        views.append((ID, (t + rng.uniform(-0.3, 0.3, 3)).astype(F), (d * rng.uniform(0.2, 5.0, (60, 1))).astype(F)))
    a = _hold(capi, DEG_PRM, views, one_call=True)
    b = _hold(capi, DEG_PRM, views, one_call=False)
    assert ocr.same_bits(a, b)
    assert not ocr.same_bits(a, ocr.integrate(DEG_PRM, ocr.empty(DEG_PRM), views[::-1])[0])
    with capi.Context() as ctx:
        ctx.occ_configure(_cparams(capi, DEG_PRM))
        arr, keep = capi.view_array(views + views[:1])
        stats = (C.c_uint64 * 4)(9, 9, 9, 9)
        assert ctx.lib.lv_occ_integrate(ctx.h, arr, 33, stats) == LV_EINVAL
        assert ctx.lib.lv_occ_integrate(ctx.h, arr, 0, stats) == LV_EINVAL
        assert list(stats) == [9, 9, 9, 9] and np.isnan(ctx.occ_fetch()).all()
    # two runs of the scene give identical bits
    r1, r2 = _run_scene(capi, scene), _run_scene(capi, scene)
    for (L1, s1), (L2, s2) in zip(r1, r2):
        assert ocr.same_bits(L1, L2) and list(s1) == list(s2)


# ---- 5. projection and query
def test_projection_and_query(capi, scene):
    prm, ref = scene["prm"], scene["after"][-1]
    rng = np.random.default_rng(6)
    lo = np.array(prm["origin"])
    hi = lo + np.array([prm["nx"], prm["ny"], prm["nz"]]) * prm["resolution"]
    q = rng.uniform(lo - 1.0, hi + 1.0, (5000, 3))
    face = rng.integers(0, 6, 5000)   # half of them within a few centimetres of a face of the grid, on either side
    for f in range(6):
        sel = (face == f) & (rng.uniform(size=5000) < 0.5)
        q[sel, f % 3] = (lo, hi)[f // 3][f % 3] + rng.normal(0.0, 0.02, sel.sum())
    # ... and the x, y of two thirds inside the room the sweeps saw, which the grid's low x and low z faces cut
    room = rng.uniform(size=5000) < 0.67
    q[room, :2] = rng.uniform((-2.75, -7.0), (7.0, 7.0), (room.sum(), 2))
    q[room, 2] = rng.uniform(-1.5, 3.0, room.sum())
    q = np.concatenate([q, [lo, hi, np.nextafter(hi.astype(F), F(-np.inf)), [np.nan, 0, 0], [0, np.inf, 0], [1e30, 0, 0]]]).astype(F)
    with capi.Context() as ctx:
        ctx.occ_configure(_cparams(capi, prm))
        ctx.occ_integrate(scene["views"])
        L = ctx.occ_fetch()
        assert ocr.same_bits(L, ref)
        for k_lo, k_hi in ((0, prm["nz"] - 1), (4, 4), (-3, 5), (20, 99), (24, 30)):   # full, one layer, clipped below / above, empty
            assert np.array_equal(ctx.occ_project(k_lo, k_hi), ocr.project(prm, ref, k_lo, k_hi)), (k_lo, k_hi)
        got = ctx.occ_query(q)
        assert ocr.same_bits(got, ocr.query(prm, L, q))
        assert np.isnan(got[-3:]).all() and np.isnan(got).sum() > 1000 and np.isfinite(got).sum() > 500
        band = ctx.occ_project(3, 5)   # z in [0.75, 2.25]: the sensors' height
        out = ctx.lib.lv_occ_project(ctx.h, 5, 3, band.ctypes.data_as(C.POINTER(C.c_int8)), C.c_size_t(band.size))
        assert out == LV_EINVAL
        assert ctx.lib.lv_occ_project(ctx.h, 3, 5, band.ctypes.data_as(C.POINTER(C.c_int8)), C.c_size_t(band.size - 1)) == LV_EINVAL
    # The wall x = +6.18 lies in column i = 15 (x in [5.75, 6.25)); the room's inside spans the rows j = 7..29 (the walls y = -+6.18
    # are rows 6 and 30).  Along the row j = 10 (y = -4), which no box touches: free from the grid's edge to the wall, the wall, unknown
    # behind it.
    assert np.all(band[8:29, 15] == 100)   # (one cell clear of both corners, where a 256-step sweep may leave a cell of the band without a return)
    assert list(band[10, :15]) == [0] * 15 and band[10, 15] == 100 and list(band[10, 16:]) == [-1] * 80
    assert (np.sum(band[10] == 0), np.sum(band[10] == 100), np.sum(band[10] == -1)) == (15, 1, 80)


# ---- 6. lifecycle
def test_lifecycle(capi, scene, tmp_path):
    from limo_velo_amd import occupancy

    prm = scene["prm"]
    with capi.Context() as ctx:
        lib, h = ctx.lib, ctx.h
        buf = np.zeros(8, F)
        fp = buf.ctypes.data_as(C.POINTER(C.c_float))
        arr, keep = capi.view_array(scene["views"][:1])
        p = capi.OccupancyParams()
        g2 = np.zeros(8, np.int8)
        assert lib.lv_occ_integrate(h, arr, 1, None) == LV_ESTATE
        assert lib.lv_occ_query(h, buf.ctypes.data_as(C.c_void_p), 12, 1, fp) == LV_ESTATE
        assert lib.lv_occ_project(h, 0, 0, g2.ctypes.data_as(C.POINTER(C.c_int8)), 8) == LV_ESTATE
        assert lib.lv_occ_fetch(h, fp, 8) == LV_ESTATE and lib.lv_occ_load(h, fp, 8) == LV_ESTATE
        assert lib.lv_occ_clear(h) == LV_ESTATE and lib.lv_occ_get_params(h, C.byref(p)) == LV_ESTATE
        bad = _cparams(capi, dict(prm, nx=1025))
        assert lib.lv_occ_configure(h, C.byref(bad)) == LV_EINVAL and lib.lv_occ_clear(h) == LV_ESTATE

        ctx.occ_configure(_cparams(capi, prm))
        assert ocr.params_of(ctx.occ_params()) == ocr.params_of(_cparams(capi, prm))
        stats = occupancy.integrate(ctx, scene["views"])
        assert list(stats) == list(np.sum(scene["stats"], axis=0))
        L = ctx.occ_fetch()
        assert ocr.same_bits(L, scene["after"][-1])
        ctx.occ_clear()
        assert np.isnan(ctx.occ_fetch()).all()
        ctx.occ_load(L)
        assert ocr.same_bits(ctx.occ_fetch(), L)
        # a wrong size, a value outside the clamp, an infinite one: refused, the grid stays
        Lbad = L.copy()
        Lbad[3, 3, 3] = 3.6
        Linf = L.copy()
        Linf[0, 0, 0] = -np.inf
        for a, n in ((L, L.size - 1), (Lbad, L.size), (Linf, L.size)):
            assert lib.lv_occ_load(h, a.ctypes.data_as(C.POINTER(C.c_float)), C.c_size_t(n)) == LV_EINVAL
        assert lib.lv_occ_fetch(h, fp, 8) == LV_EINVAL
        assert ocr.same_bits(ctx.occ_fetch(), L)
        # a refused reconfigure keeps the grid, a good one discards it
        assert lib.lv_occ_configure(h, C.byref(bad)) == LV_EINVAL and ocr.same_bits(ctx.occ_fetch(), L)
        path = str(tmp_path / "grid.npz")
        ctx.occ_load(L)
        occupancy.save_grid(ctx, path)
        grid = occupancy.occupancy_grid(ctx, 0.75, 2.25)
        ctx.occ_configure(_cparams(capi, dict(prm, nx=40)))
        assert ctx.occ_params().nx == 40 and np.isnan(ctx.occ_fetch()).all() and ctx.occ_fetch().shape == (24, 80, 40)
    assert occupancy.layers(_cparams(capi, prm), 0.75, 2.25) == (3, 5)
    assert (grid["width"], grid["height"], grid["resolution"]) == (96, 80, 0.5) and grid["origin"][:2] == (-1.75, -9.25)
    assert np.array_equal(grid["data"].reshape(80, 96), ocr.project(prm, scene["after"][-1], 3, 5))
    with capi.Context() as ctx:
        p = occupancy.load_grid(ctx, path)
        assert ocr.params_of(p) == ocr.params_of(_cparams(capi, prm)) and ocr.same_bits(ctx.occ_fetch(), L)


# ---- 7. isolation
def test_the_map_and_the_update_are_untouched(capi, scene):
    from limo_velo_amd import occupancy, synth

    sc = scene["sc"]
    with capi.Context() as ctx:
        ctx.map_build(sc["map_xyz"])
        ctx.scan_set(sc["scan_xyz"])
        x0, P0, passes0, _, _ = ctx.update(sc["x_init"], sc["P0"])
        x0, P0 = np.array(x0), np.array(P0)
        stats0 = ctx.map_stats()
        ctx.occ_configure(_cparams(capi, scene["prm"]))
        ctx.occ_integrate(scene["views"])
        states = occupancy.map_point_states(ctx)
        assert ocr.same_bits(states, ocr.query(scene["prm"], scene["after"][-1], sc["map_xyz"]))
        assert np.sum(states >= F(0.4)) > 100   # (map points sit on the surfaces the sweeps hit)
        x1, P1, passes1, _, _ = ctx.update(sc["x_init"], sc["P0"])
        assert passes1 == passes0
        assert np.array_equal(np.array(x1).view(np.uint64), x0.view(np.uint64))
        assert np.array_equal(np.array(P1).view(np.uint64), P0.view(np.uint64))
        assert ctx.map_stats() == stats0
        assert ocr.same_bits(ctx.occ_fetch(), scene["after"][-1])
