"""GPU tests of the distance field (lv_distance.hip; include/limovelo_hip.h "Distance field") against the numpy statement of the
rule in tests/distance_ref.py.  Squared distances are integers and the metres f32 operations in a stated order, so everything is
held to equality: s2 and stats as integers, metres, dist and grad as bits (NaN by isnan), no tolerance anywhere.  The grids are
set with occ_load; only the scene case integrates sweeps."""
import ctypes as C
import math

import numpy as np
import pytest

import distance_ref as dr
import occupancy_ref as ocr

pytestmark = pytest.mark.gpu

LV_EINVAL, LV_ESTATE = -1, -4
F = np.float32


@pytest.fixture(scope="module")
def capi(lv):
    from limo_velo_amd import capi as c

    return c


def _cparams(capi, prm):
    return capi.default_occupancy_params(**prm)


def _dparams(capi, dp):
    return capi.default_distance_params(**dp)


def _hold(capi, ctx, prm, L, dp, pts):
    """The GPU's field of the loaded grid L equals the reference's: s2, metres, stats, and dist / grad at pts.  Returns s2."""
    rs2, rst = dr.build(prm, L, dp)
    st = ctx.occ_distance_build(_dparams(capi, dp))
    s2, met = ctx.occ_distance_fetch()
    assert s2.shape == rs2.shape and np.array_equal(s2, rs2), (dp, f"{np.sum(s2 != rs2)} values differ")
    assert dr.same_bits(met, dr.metres(rs2, prm["resolution"])), dp
    assert list(st) == list(rst), (dp, st, rst)
    rd, rg = dr.query(prm, dp, rs2, pts)
    dist, grad = ctx.occ_distance_query(pts)
    assert dr.same_bits(dist, rd) and dr.same_bits(grad, rg), dp
    return s2


def _param_sets(nz):
    band = (1, max(nz - 2, 1))   # clipped at least at the top for nz <= 2
    return [dr.dparams(), dr.dparams(unknown_is_obstacle=1), dr.dparams(signed_field=1), dr.dparams(signed_field=1, unknown_is_obstacle=1),
            dr.dparams(max_cells=1, signed_field=1), dr.dparams(max_cells=1, unknown_is_obstacle=1), dr.dparams(max_cells=3),
            dr.dparams(max_cells=3, signed_field=1, unknown_is_obstacle=1),
            dr.dparams(planar=1, k_lo=band[0], k_hi=band[1], signed_field=1, unknown_is_obstacle=1),
            dr.dparams(planar=1, k_lo=-5, k_hi=2000), dr.dparams(planar=1, k_lo=0, k_hi=nz - 1, max_cells=3, signed_field=1)]


def _contents(rng, prm):
    nx, ny, nz = prm["nx"], prm["ny"], prm["nz"]
    corner = rng.uniform(prm["l_min"], prm["l_free"], (nz, ny, nx)).astype(F)
    corner[nz - 1, ny - 1, nx - 1] = prm["l_occ"]   # one obstacle in a corner: the longest diagonal
    return [("unknown", np.full((nz, ny, nx), np.nan, F)), ("occupied", np.full((nz, ny, nx), prm["l_max"], F)), ("corner", corner),
            ("1 %", dr.random_logodds(rng, (nz, ny, nx), 0.01, prm=prm)), ("30 %", dr.random_logodds(rng, (nz, ny, nx), 0.30, prm=prm))]


# ---- 1. shapes x contents x parameters
@pytest.mark.parametrize("dims", [(1, 5, 3), (31, 5, 3), (33, 5, 3), (65, 4, 3), (33, 1, 4), (20, 7, 1), (1, 1, 1), (1024, 2, 2), (2, 1024, 2),
                                  (70, 45, 20)])
def test_shapes_contents_and_parameters(capi, dims):
    nx, ny, nz = dims
    rng = np.random.default_rng(nx * 7 + ny * 3 + nz)
    prm = ocr.params(origin=(-1.0, 0.5, 2.0), resolution=0.25, nx=nx, ny=ny, nz=nz)
    pts = dr.probe_points(prm, rng, 40, 120)
    with capi.Context() as ctx:
        ctx.occ_configure(_cparams(capi, prm))
        for name, L in _contents(rng, prm):
            ctx.occ_load(L)
            for dp in _param_sets(nz):
                s2 = _hold(capi, ctx, prm, L, dp, pts)
                if name == "corner" and nx * ny * nz > 1 and not dp["planar"] and not dp["max_cells"] and not dp["unknown_is_obstacle"]:
                    assert s2[0, 0, 0] == (nx - 1) ** 2 + (ny - 1) ** 2 + (nz - 1) ** 2
                if name == "unknown" and not dp["unknown_is_obstacle"]:
                    assert np.all(s2 == dr.FAR)
                if name == "occupied":
                    assert np.all(s2 == (-dr.FAR if dp["signed_field"] else 0))


# ---- 2. the scene of tests/test_gpu_occupancy.py after its three sweeps
def _moved(x0, dx, dy, dyaw):
    from limo_velo_amd import synth

    x = np.array(x0, np.float64)
    x[0] += dx
    x[1] += dy
    x[3:7] = synth.quat_mul(x[3:7], synth.quat_from_rpy(0.0, 0.0, math.radians(dyaw)))
    return x


SCENE_PRM = ocr.params(origin=(-1.75, -9.25, -0.75), resolution=0.5, nx=96, ny=80, nz=24, min_range=1.0, max_range=8.0)


@pytest.fixture(scope="module")
def scene(capi):
    from limo_velo_amd import synth

    M = 20_000
    sc = synth.make_ring_scene(M, 16, 256)
    rects = synth.scene_surfaces(M)
    x0 = sc["x_true"]
    views = []
    for i, s in enumerate([x0, _moved(x0, 2.0, 1.0, 20.0), _moved(x0, -7.0, 3.5, -15.0)]):
        R, t = capi.sensor_pose(s)
        views.append((R, t, synth.ring_sweep(rects, R, t, 16, 256, range_sigma=0.01, seed=11 + i)))
    return dict(sc=sc, views=views, prm=SCENE_PRM)


def test_scene_3d_and_planar(capi, scene):
    prm = scene["prm"]
    rng = np.random.default_rng(2)
    pts = dr.probe_points(prm, rng, 100, 300)
    with capi.Context() as ctx:
        ctx.occ_configure(_cparams(capi, prm))
        ctx.occ_integrate(scene["views"])
        L = ctx.occ_fetch()
        # (what the scene is for: obstacles, observed free space and never observed space all present)
        assert np.sum(L >= F(prm["l_occ"])) > 100 and np.isnan(L).any() and np.sum(L <= F(prm["l_free"])) > 100
        for dp in (dr.dparams(), dr.dparams(signed_field=1, unknown_is_obstacle=1), dr.dparams(max_cells=6, signed_field=1),
                   dr.dparams(planar=1, k_lo=3, k_hi=5), dr.dparams(planar=1, k_lo=3, k_hi=5, signed_field=1, unknown_is_obstacle=1, max_cells=10)):
            _hold(capi, ctx, prm, L, dp, pts)
        assert ocr.same_bits(ctx.occ_fetch(), L)


# ---- 3. fetch with one output, the Python helpers
def test_fetch_outputs_and_helpers(capi):
    from limo_velo_amd import occupancy

    prm = ocr.params(origin=(-1.0, 0.5, 2.0), resolution=0.25, nx=37, ny=11, nz=6)
    rng = np.random.default_rng(9)
    L = dr.random_logodds(rng, (6, 11, 37), 0.03, prm=prm)
    dp = dr.dparams(signed_field=1)
    rs2, _ = dr.build(prm, L, dp)
    with capi.Context() as ctx:
        ctx.occ_configure(_cparams(capi, prm))
        ctx.occ_load(L)
        ctx.occ_distance_build(_dparams(capi, dp))
        s2, none = ctx.occ_distance_fetch(metres=False)
        assert none is None and np.array_equal(s2, rs2)
        none, met = ctx.occ_distance_fetch(s2=False)
        assert none is None and dr.same_bits(met, dr.metres(rs2, 0.25))
        n = rs2.size
        both = ctx.lib.lv_occ_distance_fetch(ctx.h, None, None, C.c_size_t(n))
        assert both == LV_EINVAL
        # a capacity one short: refused, nothing written
        buf = np.full(n, 77, np.int32)
        assert ctx.lib.lv_occ_distance_fetch(ctx.h, buf.ctypes.data_as(C.POINTER(C.c_int32)), None, C.c_size_t(n - 1)) == LV_EINVAL
        assert np.all(buf == 77)
        # the helpers: metres of the field; a truncated signed one; a planar one over a height band; clearance
        assert dr.same_bits(occupancy.distance_field(ctx), dr.metres(dr.build(prm, L, dr.dparams())[0], 0.25))
        got = occupancy.distance_field(ctx, max_dist=0.8, signed=True, unknown="obstacle")   # floor(0.8 / 0.25) = 3 cells
        want = dr.dparams(signed_field=1, unknown_is_obstacle=1, max_cells=3)
        assert dr.same_bits(got, dr.metres(dr.build(prm, L, want)[0], 0.25))
        i = ctx.occ_distance_info()
        assert (i.built, i.planar, i.stale, i.params.max_cells, i.params.signed_field, i.params.unknown_is_obstacle) == (1, 0, 0, 3, 1, 1)
        got = occupancy.distance_field(ctx, z_band=(2.3, 3.1))   # centres 2.375, 2.625, 2.875: the layers 1..3
        assert occupancy.layers(ctx.occ_params(), 2.3, 3.1) == (1, 3)
        want = dr.dparams(planar=1, k_lo=1, k_hi=3)
        ps2, _ = dr.build(prm, L, want)
        assert got.shape == (11, 37) and dr.same_bits(got, dr.metres(ps2, 0.25))
        pts = dr.probe_points(prm, rng, 30, 60)
        dist, grad = occupancy.clearance(ctx, pts)
        rd, rg = dr.query(prm, want, ps2, pts)
        assert dr.same_bits(dist, rd) and dr.same_bits(grad, rg) and not grad[:, 2].any()
        assert np.isfinite(dist[22]) and np.isnan(pts[22, 2])   # (the point with a NaN z is answered in a planar field)
        d_only, none = ctx.occ_distance_query(pts, want_grad=False)
        assert none is None and dr.same_bits(d_only, rd)
        # a band without a layer: no obstacles anywhere
        assert np.all(np.isposinf(occupancy.distance_field(ctx, z_band=(50.0, 51.0))))
        cost = occupancy.costmap_from_distance(got, 0.25, 0.75)
        assert cost.shape == got.shape and np.all(cost[ps2 == 0] == 254) and np.all(cost[ps2 == 1] == 253) and np.all(cost[ps2 > 9] == 0)


# ---- 4. lifecycle
def test_lifecycle(capi, scene):
    prm = ocr.params(origin=(-4.0, -4.0, -1.0), resolution=0.5, nx=34, ny=9, nz=5, min_range=0.3, max_range=8.0)
    rng = np.random.default_rng(4)
    L = dr.random_logodds(rng, (5, 9, 34), 0.05, prm=prm)
    dp = dr.dparams(signed_field=1)
    rs2, _ = dr.build(prm, L, dp)
    with capi.Context() as ctx:
        lib, h = ctx.lib, ctx.h
        info = capi.DistanceInfo()
        buf = np.zeros(8, np.int32)
        ip = buf.ctypes.data_as(C.POINTER(C.c_int32))
        fbuf = np.zeros(8, F)
        fp = fbuf.ctypes.data_as(C.POINTER(C.c_float))
        cdp = _dparams(capi, dp)
        # before lv_occ_configure
        assert lib.lv_occ_distance_build(h, C.byref(cdp), None) == LV_ESTATE
        assert lib.lv_occ_distance_fetch(h, ip, None, 8) == LV_ESTATE
        assert lib.lv_occ_distance_query(h, fbuf.ctypes.data_as(C.c_void_p), 12, 1, fp, None) == LV_ESTATE
        assert lib.lv_occ_distance_info(h, C.byref(info)) == LV_ESTATE and lib.lv_occ_distance_clear(h) == LV_ESTATE
        # configured, before a build
        ctx.occ_configure(_cparams(capi, prm))
        assert lib.lv_occ_distance_fetch(h, ip, None, 8) == LV_ESTATE
        assert lib.lv_occ_distance_query(h, fbuf.ctypes.data_as(C.c_void_p), 12, 1, fp, None) == LV_ESTATE
        i = ctx.occ_distance_info()
        assert (i.built, i.planar, i.nx, i.ny, i.nz, i.stale) == (0, 0, 0, 0, 0, 0)
        ctx.occ_distance_clear()   # (nothing to free: fine)
        ctx.occ_load(L)
        assert ctx.occ_distance_info().stale == 0   # (nothing built yet, nothing stale)
        # a refused build changes nothing
        bad = _dparams(capi, dr.dparams(max_cells=1025))
        assert lib.lv_occ_distance_build(h, C.byref(bad), None) == LV_EINVAL and ctx.occ_distance_info().built == 0
        ctx.occ_distance_build(cdp)
        i = ctx.occ_distance_info()
        assert (i.built, i.planar, i.nx, i.ny, i.nz, i.stale, i.params.signed_field) == (1, 0, 34, 9, 5, 0, 1)
        assert lib.lv_occ_distance_build(h, C.byref(bad), None) == LV_EINVAL
        assert np.array_equal(ctx.occ_distance_fetch()[0], rs2) and ctx.occ_distance_info().stale == 0
        assert lib.lv_occ_distance_fetch(h, ip, None, 8) == LV_EINVAL and not buf.any()
        # the grid moves on, the snapshot stays: after integrate, after load, after clear
        pts = dr.probe_points(prm, rng, 20, 40)
        rd, rg = dr.query(prm, dp, rs2, pts)
        t = np.array([0.1, 0.2, 0.3], F)
        ends = rng.uniform(-3.0, 3.0, (200, 3)).astype(F)
        for change in (lambda: ctx.occ_integrate([(np.eye(3, dtype=F), t, ends)]), lambda: ctx.occ_load(L), ctx.occ_clear):
            ctx.occ_load(L)
            ctx.occ_distance_build(cdp)
            assert ctx.occ_distance_info().stale == 0
            change()
            assert ctx.occ_distance_info().stale == 1 and ctx.occ_distance_info().built == 1
            assert np.array_equal(ctx.occ_distance_fetch()[0], rs2)
            dist, grad = ctx.occ_distance_query(pts)
            assert dr.same_bits(dist, rd) and dr.same_bits(grad, rg)
        # (the grid is all unknown now) a rebuild replaces the field, here by a planar one of another size
        st = ctx.occ_distance_build(_dparams(capi, dr.dparams(planar=1, k_lo=0, k_hi=4, unknown_is_obstacle=1)))
        i = ctx.occ_distance_info()
        assert (i.built, i.planar, i.nx, i.ny, i.nz, i.stale) == (1, 1, 34, 9, 1, 0) and list(st) == [34 * 9, 34 * 9, 0, 0]
        s2, met = ctx.occ_distance_fetch()
        assert s2.shape == (9, 34) and not s2.any() and not met.any()
        ctx.occ_load(L)
        ctx.occ_distance_build(cdp)
        assert np.array_equal(ctx.occ_distance_fetch()[0], rs2) and ctx.occ_distance_info().nz == 5
        # lv_occ_distance_clear discards it; so does lv_occ_configure (a refused one does not)
        ctx.occ_distance_clear()
        assert ctx.occ_distance_info().built == 0 and lib.lv_occ_distance_fetch(h, ip, None, 8) == LV_ESTATE
        ctx.occ_distance_build(cdp)
        badgrid = _cparams(capi, dict(prm, nx=1025))
        assert lib.lv_occ_configure(h, C.byref(badgrid)) == LV_EINVAL and ctx.occ_distance_info().built == 1
        ctx.occ_configure(_cparams(capi, dict(prm, nx=40)))
        assert ctx.occ_distance_info().built == 0 and lib.lv_occ_distance_fetch(h, ip, None, 8) == LV_ESTATE
        st = ctx.occ_distance_build(capi.default_distance_params())
        assert list(st) == [0, 0, 0, 0] and np.all(ctx.occ_distance_fetch()[0] == dr.FAR)


# ---- 5. untouched state
def test_the_grid_the_map_and_the_update_are_untouched(capi, scene):
    sc = scene["sc"]
    prm = scene["prm"]
    with capi.Context() as ctx:
        ctx.map_build(sc["map_xyz"])
        ctx.scan_set(sc["scan_xyz"])
        x0, P0, passes0, _, _ = ctx.update(sc["x_init"], sc["P0"])
        x0, P0 = np.array(x0), np.array(P0)
        stats0 = ctx.map_stats()
        ctx.occ_configure(_cparams(capi, prm))
        ctx.occ_integrate(scene["views"])
        before = ctx.occ_fetch()
        for dp in (dr.dparams(signed_field=1, unknown_is_obstacle=1), dr.dparams(planar=1, k_lo=3, k_hi=5, max_cells=4)):
            ctx.occ_distance_build(_dparams(capi, dp))
            ctx.occ_distance_fetch()
            ctx.occ_distance_query(sc["map_xyz"][:500])
            assert np.array_equal(ctx.occ_fetch().view(np.uint32), before.view(np.uint32))
        x1, P1, passes1, _, _ = ctx.update(sc["x_init"], sc["P0"])
        assert passes1 == passes0
        assert np.array_equal(np.array(x1).view(np.uint64), x0.view(np.uint64))
        assert np.array_equal(np.array(P1).view(np.uint64), P0.view(np.uint64))
        assert ctx.map_stats() == stats0
