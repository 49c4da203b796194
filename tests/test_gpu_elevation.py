"""lv_elev_* and lv_occ_distance_build_cells (include/limovelo_hip.h "Elevation map") on the GPU, through capi and terrain.py,
against tests/elevation_ref.py: equality on every layer, the class grid, the stats and the queries, no tolerance.  The cases of
tests/test_elevation_host.py and its 70 x 37 scene from caller points; the scene through the device map with a slab evicted; one
cell and a few cells under heavy contention; ragged and empty launches; builds of changing size on one context; queries; an
unbuilt map; the distance field from cells against the one from the projected grid; and the chain from the class grid through
the distance field to the planner."""
import ctypes as C

import numpy as np
import pytest

import distance_ref as dr
import elevation_cases as cases
import elevation_ref as er
import occ_ray_cases as ray_cases
import occupancy_ref as ocr

pytestmark = pytest.mark.gpu

LV_OK, LV_EINVAL, LV_ESTATE = 0, -1, -4
F = np.float32


@pytest.fixture(scope="module")
def capi(lv):
    from limo_velo_amd import capi as c

    return c


def _params(capi, prm):
    return capi.default_elevation_params(**prm)


def _layers(capi, ctx):
    return {name: ctx.elev_fetch(layer) for layer, (name, _) in enumerate(capi.ELEV_LAYERS)}


def _held(capi, ctx, stats, want, what):
    got = _layers(capi, ctx)
    assert er.same_layers(got, want[0]) is None, (what, er.same_layers(got, want[0]))
    assert stats.dtype == np.uint64 and np.array_equal(stats, want[1]), (what, stats, want[1])


def test_cases_and_scene_from_caller_points(capi):
    from limo_velo_amd import terrain

    want = cases.answers()
    with capi.Context() as ctx:
        for name, (prm, pts) in cases.cases().items():
            _held(capi, ctx, ctx.elev_build(_params(capi, prm), pts), want[name], name)
        prm, pts = cases.scene_params(), cases.scene()
        out = terrain.elevation(ctx, _params(capi, prm), pts)
        L, stats = cases.scene_answer()
        assert er.same_layers(out, L) is None and np.array_equal(out["stats"], stats)
        assert np.array_equal(terrain.traversability(ctx, _params(capi, prm), pts), L["cls"])
        i = ctx.elev_info()
        assert (i.built, i.nx, i.ny, i.from_map, i.n_points) == (1, 70, 37, 0, len(pts)) and bytes(i.params) == bytes(_params(capi, prm))
        # a strided array: the first three floats of every 20 bytes
        wide = np.zeros((len(pts), 5), F)
        wide[:, :3] = pts
        wide[:, 3:] = np.nan
        st = np.zeros(4, np.uint64)
        p = _params(capi, prm)
        assert ctx.lib.lv_elev_build(ctx.h, C.byref(p), wide.ctypes.data, 20, len(wide), st.ctypes.data_as(C.POINTER(C.c_uint64))) == LV_OK
        _held(capi, ctx, st, (L, stats), "strided")
        assert ctx.lib.lv_elev_build(ctx.h, C.byref(p), wide.ctypes.data, 20, len(wide), None) == LV_OK   # (stats may be NULL)


def test_map_source_skips_dead_ids_and_order_does_not_matter(capi):
    prm, pts = cases.scene_params(), cases.scene()
    p = _params(capi, prm)
    with capi.Context() as ctx:
        ctx.map_build(pts)
        gone = ctx.map_evict_box((-0.5, -3.7, -5.0), (2.1, -0.9, 5.0), keep_inside=False)   # a slab with the table in it
        assert gone > 3000 and ctx.map_size() == len(pts) - gone
        stats = ctx.elev_build(p, None)
        living = ctx.map_fetch()
        want = er.build(prm, living)
        _held(capi, ctx, stats, want, "map")
        i = ctx.elev_info()
        assert (i.built, i.from_map, i.n_points) == (1, 1, len(living))
        assert stats[0] == len(living) and np.any(want[0]["cls"] != cases.scene_answer()[0]["cls"]) and (want[0]["count"] == 0).sum() > 100
        # a snapshot: the map moves on, the elevation map does not
        ctx.map_evict_box((-7.0, -3.7, -5.0), (0.0, 3.7, 5.0), keep_inside=False)
        ctx.map_add(pts[:500])
        _held(capi, ctx, stats, want, "snapshot")
        # the same set as caller points, reversed
        with capi.Context() as other:
            _held(capi, other, other.elev_build(p, living[::-1]), want, "reversed")
            assert other.elev_info().from_map == 0


def test_contention(capi):
    rng = np.random.default_rng(8)
    with capi.Context() as ctx:
        prm = er.params(origin=(0.0, 0.0, 0.0), resolution=1.0, nx=1, ny=1, min_points=3, head=300, max_span=2 ** 25, max_step=0, max_slope2=0)
        pts = np.column_stack([rng.uniform(0, 1, (5000, 2)), rng.uniform(-2.0, 2.0, 5000)]).astype(F)
        want = er.build(prm, pts)
        _held(capi, ctx, ctx.elev_build(_params(capi, prm), pts), want, "1 x 1")
        assert want[0]["count"][0, 0] == 5000 and 0 < want[0]["band_count"][0, 0] < 5000 and want[1][1] > 0
        prm = er.params(origin=(-3.0, 1.0, 0.5), resolution=0.25, nx=257, ny=9, min_points=44, head=200, max_span=85, max_step=90, max_slope2=20000)
        i, j = np.meshgrid(np.arange(257), np.arange(9))
        ij = np.repeat(np.column_stack([i.ravel(), j.ravel()]), 64, axis=0)
        xy = np.array([-3.0, 1.0]) + (ij + rng.uniform(0.02, 0.98, ij.shape)) * 0.25
        z = 0.5 + 0.02 * ij[:, 0] + rng.choice([0.0, 0.0, 0.05, 0.5], len(ij)) + rng.normal(0, 0.01, len(ij))
        pts = np.column_stack([xy, z])[rng.permutation(len(ij))].astype(F)
        want = er.build(prm, pts)
        _held(capi, ctx, ctx.elev_build(_params(capi, prm), pts), want, "257 x 9")
        assert np.all(want[0]["count"] == 64) and want[1][1] > 1000 and 0 < want[1][2] < 257 * 9 and 0 < want[1][3] < want[1][2]


def test_ragged_and_empty_launches(capi):
    prm, pts = cases.cases()["random"]
    with capi.Context() as ctx:
        for n in (1, 63, 65, 255, 257, 1001):
            _held(capi, ctx, ctx.elev_build(_params(capi, prm), pts[:n]), er.build(prm, pts[:n]), n)
        stats = ctx.elev_build(_params(capi, prm), pts[:0])
        L = _layers(capi, ctx)
        _held(capi, ctx, stats, er.build(prm, pts[:0]), 0)
        assert not stats.any() and np.all(L["cls"] == -1) and np.all(np.isnan(L["height"])) and np.all(L["lo"] == er.NONE) and np.all(L["top"] == -er.NONE)
        assert ctx.elev_info().n_points == 0


def test_repeated_builds_reinitialise_and_touch_nothing_else(capi):
    rng = np.random.default_rng(21)
    occ_prm = ocr.params(origin=(-3.0, -2.0, -0.5), resolution=0.1, nx=70, ny=37, nz=11, min_range=0.2, max_range=5.0)
    Lg = np.array([np.nan, -1.0, 1.0], F)[rng.choice(3, size=(11, 37, 70), p=(0.3, 0.6, 0.1))]
    map_pts = cases.scene()[:5000]

    def cloud(nx, ny, res, n):
        return np.column_stack([rng.uniform(-0.2, nx * res + 0.2, n), rng.uniform(-0.2, ny * res + 0.2, n),
                                rng.choice([0.0, 0.08, 0.6, 3.0], n) + rng.normal(0, 0.02, n)]).astype(F)

    builds = [(er.params(origin=(0.0, 0.0, -1.0), resolution=0.25, nx=300, ny=200, min_points=1, head=1000, max_span=100, max_step=60, max_slope2=8000), 30000),
              (er.params(origin=(0.0, 0.0, -1.0), resolution=0.5, nx=19, ny=13, min_points=2, head=100, max_span=30, max_step=200, max_slope2=90000), 900),
              (er.params(origin=(0.0, 0.0, -2.0), resolution=0.2, nx=400, ny=250, min_points=1, head=2000, max_span=80, max_step=20, max_slope2=400), 20000)]
    with capi.Context() as ctx:
        ctx.map_build(map_pts)
        ctx.occ_configure(capi.default_occupancy_params(**occ_prm))
        ctx.occ_load(Lg)
        ctx.occ_distance_build(capi.default_distance_params(signed_field=1))
        s2, living = ctx.occ_distance_fetch()[0], ctx.map_fetch()
        for prm, n in builds:
            pts = cloud(prm["nx"], prm["ny"], prm["resolution"], n)
            stats = ctx.elev_build(_params(capi, prm), pts)
            got = _layers(capi, ctx)
            with capi.Context() as fresh:
                fstats = fresh.elev_build(_params(capi, prm), pts)
                assert er.same_layers(got, _layers(capi, fresh)) is None and np.array_equal(stats, fstats)
            want = er.build(prm, pts)
            assert er.same_layers(got, want[0]) is None and np.array_equal(stats, want[1]), (prm["nx"], er.same_layers(got, want[0]))
            assert 0 < want[1][3] < want[1][2] < prm["nx"] * prm["ny"]
        assert ocr.same_bits(ctx.occ_fetch(), Lg) and np.array_equal(ctx.occ_distance_fetch()[0], s2) and ctx.occ_distance_info().stale == 0
        assert len(living) == len(map_pts) and np.array_equal(ctx.map_fetch().view(np.uint32), living.view(np.uint32))
        # a refused build leaves the last one in place; a cleared one is gone
        bad = _params(capi, dict(builds[0][0], nx=0))
        assert ctx.lib.lv_elev_build(ctx.h, C.byref(bad), map_pts.ctypes.data, 12, 10, None) == LV_EINVAL
        assert er.same_layers(_layers(capi, ctx), want[0]) is None and ctx.elev_info().nx == 400
        buf = np.zeros(400 * 250, np.int32)
        assert ctx.lib.lv_elev_fetch(ctx.h, capi.LV_ELEV_LO, buf.ctypes.data, 400 * 250 - 1) == LV_EINVAL and not buf.any()
        assert ctx.lib.lv_elev_fetch(ctx.h, 9, buf.ctypes.data, buf.size) == LV_EINVAL and not buf.any()
        ctx.elev_clear()
        assert ctx.elev_info().built == 0 and ctx.lib.lv_elev_fetch(ctx.h, capi.LV_ELEV_LO, buf.ctypes.data, buf.size) == LV_ESTATE


def test_query(capi):
    from limo_velo_amd import terrain

    prm, pts = cases.scene_params(), cases.scene()
    L, _ = cases.scene_answer()
    rng = np.random.default_rng(3)
    i, j = np.meshgrid(np.arange(70), np.arange(37))
    centres = np.column_stack([-7.0 + (i.ravel() + 0.5) * 0.2, -3.7 + (j.ravel() + 0.5) * 0.2, rng.normal(size=i.size)])
    borders = np.column_stack([-7.0 + i.ravel() * 0.2, -3.7 + j.ravel() * 0.2, np.zeros(i.size)])
    odd = np.array([[-7.0, -3.7, np.nan], [np.nan, 0, 0], [0, np.inf, 0], [6.9999, 3.6999, -np.inf], [-7.0001, 0, 0], [1e30, 0, 0], [7.0, 0, 0],
                    [0, 3.7001, 0], [0, -np.inf, 0]])
    q = np.vstack([centres, borders, odd, np.column_stack([rng.uniform(-7.5, 7.5, 333), rng.uniform(-4.2, 4.2, 333), np.zeros(333)])]).astype(F)
    with capi.Context() as ctx:
        ctx.elev_build(_params(capi, prm), pts)
        h, k = ctx.elev_query(q)
        wh, wk = er.query(prm, L, q)
        assert er.same_bits(h, wh) and np.array_equal(k, wk)
        assert er.same_bits(h[:i.size].reshape(37, 70), L["height"]) and np.array_equal(k[:i.size].reshape(37, 70), L["cls"])
        n0 = 2 * i.size
        assert not np.isnan(h[n0]) and np.all(np.isnan(h[[n0 + 1, n0 + 2, n0 + 4, n0 + 5, n0 + 6, n0 + 7, n0 + 8]])) and np.all(k[[n0 + 1, n0 + 4, n0 + 6]] == -1)
        # either output alone
        h1 = np.zeros(len(q), F)
        k1 = np.zeros(len(q), np.int8)
        assert ctx.lib.lv_elev_query(ctx.h, q.ctypes.data, 12, len(q), h1.ctypes.data_as(C.POINTER(C.c_float)), None) == LV_OK
        assert ctx.lib.lv_elev_query(ctx.h, q.ctypes.data, 12, len(q), None, k1.ctypes.data_as(C.POINTER(C.c_int8))) == LV_OK
        assert er.same_bits(h1, wh) and np.array_equal(k1, wk)
        assert ctx.lib.lv_elev_query(ctx.h, None, 0, 0, h1.ctypes.data_as(C.POINTER(C.c_float)), None) == LV_OK
        g = terrain.ground_points(ctx, [[0.0, 0.0], [5.0, 0.0], [-1.3, -2.5], [100.0, 0.0]])
        assert g.shape == (4, 3) and abs(g[0, 2]) < 0.02 and 0.35 < g[1, 2] < 0.45 and np.isnan(g[2, 2]) and np.isnan(g[3, 2])


def test_unbuilt_map_and_states(capi):
    prm = cases.prm()
    p = _params(capi, prm)
    with capi.Context() as ctx:
        buf = np.full(19 * 13, 7, np.int32)
        h = np.full(2, 7, np.int8)
        pts = np.zeros((2, 3), F)
        assert ctx.elev_info().built == 0
        assert ctx.lib.lv_elev_fetch(ctx.h, capi.LV_ELEV_LO, buf.ctypes.data, buf.size) == LV_ESTATE
        assert ctx.lib.lv_elev_query(ctx.h, pts.ctypes.data, 12, 2, None, h.ctypes.data_as(C.POINTER(C.c_int8))) == LV_ESTATE
        assert np.all(buf == 7) and np.all(h == 7)
        ctx.elev_clear()   # (nothing to free: fine)
        stats = ctx.elev_build(p, None)   # no map yet
        L = _layers(capi, ctx)
        assert not stats.any() and np.all(L["cls"] == -1) and np.all(L["count"] == 0) and np.all(np.isnan(L["height"]))
        _held(capi, ctx, stats, er.build(prm, np.zeros((0, 3), F)), "no map")
        i = ctx.elev_info()
        assert (i.built, i.from_map, i.n_points, i.nx, i.ny) == (1, 1, 0, 19, 13)
        # a map emptied again reads the same
        ctx.map_build(cases.cases()["random"][1])
        assert ctx.elev_build(p, None)[0] > 0
        ctx.map_evict_box((-100, -100, -100), (100, 100, 100), keep_inside=False)
        assert ctx.map_size() == 0 and not ctx.elev_build(p, None).any() and np.all(ctx.elev_fetch(capi.LV_ELEV_CLASS) == -1)
        # the distance field from cells wants a configured grid
        cells = np.zeros(19 * 13, np.int8)
        d = capi.default_distance_params(planar=1)
        assert ctx.lib.lv_occ_distance_build_cells(ctx.h, C.byref(d), cells.ctypes.data_as(C.POINTER(C.c_int8)), cells.size, None) == LV_ESTATE


@pytest.fixture(scope="module")
def integrated():
    """The 70 x 37 x 11 grid of tests/test_gpu_occ_ray.py, as three views leave it."""
    prm = ocr.params(origin=(-3.0, -2.0, -0.5), resolution=0.1, nx=70, ny=37, nz=11, min_range=0.2, max_range=5.0)
    rng = np.random.default_rng(12)

    def view(t, n, far):
        d = rng.normal(size=(n, 3))
        d /= np.linalg.norm(d, axis=1)[:, None]
        return ray_cases._rot(rng), np.asarray(t, F), (d * rng.uniform(0.15, far, (n, 1))).astype(F)

    sweeps = [view((-1.0, -0.5, 0.0), 700, 3.0), view((2.5, 1.0, 0.3), 700, 3.0), view((0.3, -2.4, 0.1), 500, 6.0)]
    return prm, ocr.integrate(prm, ocr.empty(prm), sweeps)[0]


def test_distance_from_cells_is_the_planar_field(capi, integrated):
    prm, L = integrated
    with capi.Context() as ctx:
        ctx.occ_configure(capi.default_occupancy_params(**prm))
        ctx.occ_load(L)
        k_lo, k_hi = 3, 7
        cells = ctx.occ_project(k_lo, k_hi)
        assert all((cells == v).sum() > 20 for v in (100, 0, -1))
        for unknown in (0, 1):
            for signed in (0, 1):
                for max_cells in (0, 5):
                    kw = dict(planar=1, unknown_is_obstacle=unknown, signed_field=signed, max_cells=max_cells)
                    a = ctx.occ_distance_build(capi.default_distance_params(k_lo=k_lo, k_hi=k_hi, **kw))
                    want, wm = ctx.occ_distance_fetch()
                    ctx.occ_distance_clear()
                    b = ctx.occ_distance_build_cells(cells, capi.default_distance_params(k_lo=9, k_hi=-4, **kw))
                    got, gm = ctx.occ_distance_fetch()
                    assert np.array_equal(got, want) and np.array_equal(a, b) and er.same_bits(gm, wm), kw
                    i = ctx.occ_distance_info()
                    assert (i.built, i.planar, i.nx, i.ny, i.nz, i.stale, i.params.k_lo, i.params.k_hi) == (1, 1, 70, 37, 1, 0, 9, -4)
        # every other value is not an obstacle: 50, 1, 99 never, -2 with unknown_is_obstacle only
        odd = cells.copy()
        odd[cells == 0] = np.resize(np.array([50, 1, 99, 0], np.int8), (cells == 0).sum())
        odd[cells == -1] = np.resize(np.array([-2, -1, -128], np.int8), (cells == -1).sum())
        for unknown in (0, 1):
            ctx.occ_distance_build_cells(cells, capi.default_distance_params(planar=1, unknown_is_obstacle=unknown))
            want = ctx.occ_distance_fetch()[0]
            ctx.occ_distance_build_cells(odd, capi.default_distance_params(planar=1, unknown_is_obstacle=unknown))
            got = ctx.occ_distance_fetch()[0]
            assert np.array_equal(got, want) and np.array_equal(got == 0, er.distance_cells_obstacles(odd, unknown))
            assert np.array_equal(got, dr.field(er.distance_cells_obstacles(odd, unknown)[None], dr.dparams(planar=1, unknown_is_obstacle=unknown))[0])
        # the stale rule is the field's: the grid moves on, the field stays and says so; the query and the planner read it
        ctx.occ_plan_build(np.array([[0.0, 0.0, 0.0]], F), np.array([200, 90, 50], np.uint8), capi.default_plan_params())
        ctx.occ_load(L)
        assert ctx.occ_distance_info().stale == 1 and np.array_equal(ctx.occ_distance_fetch()[0], got)
        # refusals that need the grid: they leave the old field in place
        st = np.full(4, 7, np.uint64)
        d = capi.default_distance_params(planar=1)
        Cp = cells.ctypes.data_as(C.POINTER(C.c_int8))
        assert ctx.lib.lv_occ_distance_build_cells(ctx.h, C.byref(d), Cp, cells.size - 1, st.ctypes.data_as(C.POINTER(C.c_uint64))) == LV_EINVAL
        assert ctx.lib.lv_occ_distance_build_cells(ctx.h, C.byref(d), Cp, cells.size * 11, st.ctypes.data_as(C.POINTER(C.c_uint64))) == LV_EINVAL
        d0 = capi.default_distance_params(planar=0)
        assert ctx.lib.lv_occ_distance_build_cells(ctx.h, C.byref(d0), Cp, cells.size, st.ctypes.data_as(C.POINTER(C.c_uint64))) == LV_EINVAL
        assert np.all(st == 7) and np.array_equal(ctx.occ_distance_fetch()[0], got) and ctx.occ_distance_info().stale == 1
        assert ctx.occ_plan_info().stale == 0   # (no field was built: the plan still shows the last one)


def test_chain_from_terrain_to_routes(capi):
    from limo_velo_amd import occupancy, terrain

    pts = cases.scene()
    L, _ = cases.scene_answer()
    with capi.Context() as ctx:
        ctx.occ_configure(capi.default_occupancy_params(origin=cases.SCENE_ORIGIN, resolution=cases.SCENE_RES, nx=70, ny=37, nz=4))
        p = terrain.like_occupancy(ctx)
        assert bytes(p) == bytes(_params(capi, cases.scene_params()))
        cls = terrain.traversability(ctx, p, pts)
        assert np.array_equal(cls, L["cls"]) and np.all(L["cls"][:, cases.WALL_I] == 100)   # the wall column is lethal in every row
        # merged with the (empty: all unknown) occupancy projection nothing changes; with an occupied voxel that cell turns lethal
        assert np.array_equal(terrain.traversability(ctx, p, pts, z_band=(-1.0, -0.2)), cls)
        grid = np.full((4, 37, 70), np.nan, F)
        grid[1, 18, 40] = 1.0
        ctx.occ_load(grid)
        merged = terrain.traversability(ctx, p, pts, z_band=(-1.0, -0.2))
        assert cls[18, 40] == 0 and merged[18, 40] == 100 and (merged != cls).sum() == 1
        metres = terrain.distance_field(ctx, cls)
        assert metres.shape == (37, 70) and np.all(metres[:, cases.WALL_I] == 0) and np.array_equal(metres == 0, cls == 100)
        start = terrain.ground_points(ctx, [[0.0, 0.0]])
        goals = terrain.ground_points(ctx, [[5.0, 0.0], [-5.0, 0.0]])
        assert abs(start[0, 2]) < 0.02 and 0.35 < goals[0, 2] < 0.45 and abs(goals[1, 2]) < 0.02
        occupancy.plan(ctx, goals[:1], 0.2)
        (line, status, cost), = occupancy.routes(ctx, start)
        assert status == 0 and len(line) >= 25 and cost < capi.LV_PLAN_UNREACHED
        ij = np.floor((line[:, :2] - np.array(cases.SCENE_ORIGIN[:2])) / cases.SCENE_RES).astype(int)
        assert np.all(cls[ij[:, 1], ij[:, 0]] == 0) and tuple(ij[0]) == cases.scene_cell(0.0, 0.0) and tuple(ij[-1]) == cases.scene_cell(5.0, 0.0)
        d, _ = occupancy.clearance(ctx, np.column_stack([line[:, :2], np.zeros(len(line))]).astype(F))
        assert np.all(d >= 0.2)
        occupancy.plan(ctx, goals[1:], 0.2)
        (line, status, cost), = occupancy.routes(ctx, start)
        assert status == 1 and len(line) == 0 and cost == capi.LV_PLAN_UNREACHED
