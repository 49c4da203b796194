"""GPU tests of lv_occ_from_surface (lv_surf_occ.hip; include/limovelo_hip.h "Occupancy from the surface") against the numpy
statement of the rule in tests/surf_occ_ref.py, by EQUALITY on every bit of the grid and on all four stats: one f32 step, integers
after it, so there is no tolerance and no undecided share.  The scene is tests/surf_occ_cases.py's, loaded with lv_tsdf_load
(tests/test_surf_occ_ref.py holds that every combination reaches every class)."""
import numpy as np
import pytest

import surf_occ_cases as sc
import surf_occ_ref as sr

pytestmark = pytest.mark.gpu

F = np.float32


@pytest.fixture(scope="module")
def capi(lv):
    from limo_velo_amd import capi as c

    return c


@pytest.fixture(scope="module")
def vol():
    return sc.volume()


def _occ_params(capi, name=None, **kw):
    g = dict(sc.GRIDS[name]) if name else {}
    g.update(kw)
    nz, ny, nx = g["shape"]
    return capi.default_occupancy_params(origin=[float(v) for v in g["origin"]], resolution=g["resolution"], nx=nx, ny=ny, nz=nz)


def _open(capi, vol, name=None, load=True, **kw):
    """a context with the scene's volume (loaded unless told otherwise) and the named grid, every voxel unknown"""
    ctx = capi.Context()
    ctx.tsdf_configure(capi.default_tsdf_params(origin=list(sc.ORIGIN), resolution=sc.RES, nx=sc.NX, ny=sc.NY, nz=sc.NZ, trunc_cells=sc.TRUNC_CELLS,
                                                max_weight=sc.MAX_WEIGHT))
    if load:
        ctx.tsdf_load(*vol)
    if name or kw:
        ctx.occ_configure(_occ_params(capi, name, **kw))
    return ctx


def _geometries(ctx):
    o, t = ctx.occ_params(), ctx.tsdf_params()
    return (sr.geometry(list(o.origin), o.resolution, (o.nz, o.ny, o.nx)), sr.geometry(list(t.origin), t.resolution, (t.nz, t.ny, t.nx)))


def _call(capi, ctx, S, W, L, what, **kw):
    """One lv_occ_from_surface on ctx, whose grid holds L, held to the reference of that call; returns (the grid after, stats)."""
    grid, v = _geometries(ctx)
    st = ctx.occ_from_surface(capi.default_occ_surface_params(**kw))
    got = ctx.occ_fetch()
    want, wst = sr.from_surface(L, grid, v, S, W, sc.L_MIN, sc.L_MAX, **kw)
    diff = int((got.view(np.uint32) != want.view(np.uint32)).sum())
    print(f"{what}: stats {st} (reference {wst}), {diff} voxels differ")
    assert np.array_equal(st, wst), (what, st, wst)
    assert diff == 0, what
    return got, st


def _unknown(shape):
    return np.full(shape, sr.NAN_BITS.view(F), F)


@pytest.mark.parametrize("name", list(sc.GRIDS))
def test_the_27_combinations(capi, vol, name):
    with _open(capi, vol, name) as ctx:
        shape = sc.GRIDS[name]["shape"]
        for mw, band in sc.WEIGHT_BANDS:
            for reach in sc.REACHES:
                ctx.occ_clear()
                _, st = _call(capi, ctx, *vol, _unknown(shape), f"{name} min_weight {mw} band {band} reach {reach}", min_weight=mw, band=band, reach=reach,
                              mode=sr.REPLACE)
                assert st[0] >= 84 and st[1] >= 84 and st[2] == st[0] + st[1]
                assert (st[3] > 3000) == (name == "coarse")


@pytest.mark.parametrize("mode", [sr.FILL, sr.OVERWRITE, sr.REPLACE, sr.ACCUMULATE])
def test_the_four_modes_and_boxes(capi, vol, mode):
    nz, ny, nx = sc.GRIDS["fine"]["shape"]
    L = sc.random_grid((nz, ny, nx), 21)
    boxes = (((0, 0, 0), (1 << 30,) * 3), ((7, 5, 2), (nx - 9, ny - 6, nz - 3)), ((-4, -1, -9), (nx + 2, ny, nz + 5)))
    with _open(capi, vol, "fine") as ctx:
        for lo, hi in boxes:
            ctx.occ_load(L)
            got, st = _call(capi, ctx, *vol, L, f"mode {mode} box {lo}..{hi}", lo=lo, hi=hi, reach=1, band=64, mode=mode, l_solid=0.9, l_open=-0.7)
            assert st[2] > 100
            out = np.ones(L.shape, bool)
            out[sr.clip_box(L.shape, lo, hi)] = False   # (the reference holds it too; said once more: outside the box nothing moves)
            assert np.array_equal(got[out].view(np.uint32), L[out].view(np.uint32))
        ctx.occ_load(L)
        _call(capi, ctx, *vol, L, f"mode {mode}, beyond the clamps", mode=mode, l_solid=9.0, l_open=-9.0)


@pytest.mark.parametrize("shape,origin", [((40, 90, 300), (-1.2, -2.1, -0.6)), ((100, 100, 60), (6.0, -2.3, -2.0))])
def test_grids_beyond_one_pass_of_the_workgroups(capi, vol, shape, origin):
    """At 0.06 m.  300 x 90 x 40 over the whole volume: 1.08 M voxels, five wavefront steps along a row.  60 x 100 x 100 round the
    wall: a row shorter than a wavefront, and 10 000 rows, more than 2048 workgroups x 4 wavefronts, so the write pass strides."""
    with _open(capi, vol, origin=origin, resolution=0.06, shape=shape) as ctx:
        _, st = _call(capi, ctx, *vol, _unknown(shape), f"{shape}", mode=sr.REPLACE, reach=2)
        assert st[0] > 5000 and st[1] > 5000 and st[3] > 5000
        L = ctx.occ_fetch()
        _, st = _call(capi, ctx, *vol, L, f"{shape} again", mode=sr.REPLACE, reach=2)
        assert st[2] == 0


def test_both_volumes_recentred(capi, vol):
    from colour_ref import shift_layer

    dv, dg = (3, -2, 1), (-5, 4, 0)
    with _open(capi, vol, "coarse") as ctx:
        ctx.volume_recentre(capi.LV_VOLUME_SURFACE, dv)
        ctx.volume_recentre(capi.LV_VOLUME_OCC, dg)
        grid, v = _geometries(ctx)
        assert [F(x) for x in grid["origin"]] == sr.origin_at(sc.GRIDS["coarse"]["origin"], dg, sc.GRIDS["coarse"]["resolution"])
        assert [F(x) for x in v["origin"]] == sr.origin_at(sc.ORIGIN, dv, sc.RES)
        now = ctx.tsdf_fetch()
        assert np.array_equal(now["S"], shift_layer(vol[0], dv)) and np.array_equal(now["W"], shift_layer(vol[1], dv))
        L = sc.random_grid(grid["shape"], 22)
        for mode in (sr.REPLACE, sr.FILL):
            ctx.occ_load(L)
            _, st = _call(capi, ctx, now["S"], now["W"], L, f"recentred, mode {mode}", mode=mode, reach=3)
            assert st[0] > 100 and st[1] > 100 and st[3] > 1000
        # the origins of before give another grid: the centres did move
        stay, _ = sr.from_surface(L, sc.grid_geometry("coarse"), sc.vol_geometry(), now["S"], now["W"], mode=sr.FILL, reach=3)
        assert not np.array_equal(stay.view(np.uint32), ctx.occ_fetch().view(np.uint32))


def test_empty_and_degenerate_cases(capi, vol):
    S, W = vol
    shape = sc.GRIDS["same"]["shape"]
    L = sc.random_grid(shape, 23)
    observed = int((L.view(np.uint32) != sr.NAN_BITS).sum())
    with _open(capi, vol, "same", load=False) as ctx:   # a never observed volume
        ctx.occ_load(L)
        _, st = _call(capi, ctx, 0 * S, 0 * W, L, "never observed, ACCUMULATE", mode=sr.ACCUMULATE, reach=4)
        assert not st.any()
        got, st = _call(capi, ctx, 0 * S, 0 * W, L, "never observed, REPLACE", mode=sr.REPLACE, reach=4)
        assert list(st) == [0, 0, observed, 0] and (got.view(np.uint32) == sr.NAN_BITS).all()
    with _open(capi, vol, "same") as ctx:
        ctx.occ_load(L)
        _, st = _call(capi, ctx, S, W, L, "min_weight above every W", mode=sr.OVERWRITE, min_weight=6)
        assert not st.any()
        got, st = _call(capi, ctx, S, W, L, "band 4096", mode=sr.REPLACE, band=4096)
        assert st[0] == (W > 0).sum() and st[1] == 0
        _, st = _call(capi, ctx, S, W, got, "band -4096", mode=sr.REPLACE, band=-4096)
        assert st[0] == 0 and st[1] == (W > 0).sum() and st[2] == st[1]
        got, st = _call(capi, ctx, S, W, ctx.occ_fetch(), "an empty box", mode=sr.REPLACE, lo=(5, 5, 5), hi=(4, 9, 9))
        assert not st.any()
    # grids that do not overlap the volume: beside it, 65536 voxels and more away (the centre does not quantise), and beyond f32's reach
    for origin in ((100.0, 0.0, 0.0), (0.0, -3.0e4, 0.0), (0.0, 0.0, 1.0e30)):
        with _open(capi, vol, origin=origin, resolution=0.4, shape=(3, 4, 5)) as ctx:
            Lf = sc.random_grid((3, 4, 5), 24)
            ctx.occ_load(Lf)
            _, st = _call(capi, ctx, S, W, Lf, f"far grid {origin}, FILL", mode=sr.FILL, reach=4)
            assert list(st) == [0, 0, 0, 60]
            got, st = _call(capi, ctx, S, W, Lf, f"far grid {origin}, REPLACE", mode=sr.REPLACE, reach=4)
            assert st[3] == 60 and st[2] > 20 and (got.view(np.uint32) == sr.NAN_BITS).all()


def test_the_stale_rule_and_the_surface_side(capi, vol):
    S, W = vol
    rng = np.random.default_rng(25)
    with _open(capi, vol, "same") as ctx:
        Wc = rng.integers(0, 5, S.shape + (1,))
        C4 = np.concatenate([rng.integers(0, 256, S.shape + (3,)) * Wc, Wc], axis=-1).astype(np.uint32)
        ctx.colour_load(C4)
        ctx.tsdf_mesh_build(1)
        ctx.occ_distance_build()
        ctx.occ_frontier_build()
        assert ctx.occ_distance_info().stale == 0 and ctx.occ_frontier_info().stale == 0 and ctx.tsdf_mesh_info().stale == 0
        kw = dict(mode=sr.REPLACE, reach=1)
        _, st = _call(capi, ctx, S, W, _unknown(S.shape), "first REPLACE", **kw)
        assert st[2] > 0 and ctx.occ_distance_info().stale == 1 and ctx.occ_frontier_info().stale == 1   # GRID EDIT
        ctx.occ_distance_build()
        ctx.occ_frontier_build()
        _, st = _call(capi, ctx, S, W, ctx.occ_fetch(), "the same REPLACE again", **kw)
        assert st[2] == 0 and st[0] > 0 and ctx.occ_distance_info().stale == 0 and ctx.occ_frontier_info().stale == 0   # nothing changed: nothing stale
        # the surface side: not a bit, and no mark
        after = ctx.tsdf_fetch()
        assert np.array_equal(after["S"], S) and np.array_equal(after["W"], W) and np.array_equal(ctx.colour_fetch()["sums"], C4)
        assert ctx.tsdf_mesh_info().stale == 0
        # a refused call changes nothing and marks nothing
        before = ctx.occ_fetch()
        with pytest.raises(capi.LvError, match="error -1: lv_occ_from_surface: reach = 5"):
            ctx.occ_from_surface(capi.default_occ_surface_params(reach=5, mode=sr.ACCUMULATE))
        assert np.array_equal(ctx.occ_fetch().view(np.uint32), before.view(np.uint32)) and ctx.occ_distance_info().stale == 0


def test_states(capi, vol):
    with capi.Context() as ctx:
        with pytest.raises(capi.LvError, match="error -4: no occupancy grid"):
            ctx.occ_from_surface()
        with pytest.raises(capi.LvError, match="error -1: lv_occ_from_surface: mode = 7"):   # the parameters come first
            ctx.occ_from_surface(capi.default_occ_surface_params(mode=7))
        ctx.occ_configure(_occ_params(capi, "same"))
        with pytest.raises(capi.LvError, match="error -4: no TSDF volume"):
            ctx.occ_from_surface()
        with pytest.raises(capi.LvError, match="error -4: no TSDF volume"):   # ... and the states before the box
            ctx.occ_from_surface(capi.default_occ_surface_params(lo=(5, 5, 5), hi=(4, 9, 9)))
        assert np.isnan(ctx.occ_fetch()).all()
    with _open(capi, vol) as ctx:   # a volume and no grid: the grid is asked for first
        with pytest.raises(capi.LvError, match="error -4: no occupancy grid"):
            ctx.occ_from_surface()
    with _open(capi, vol, "same") as ctx:   # a new grid starts over: the bitmaps are allocated again by the next call
        _call(capi, ctx, *vol, _unknown(sc.GRIDS["same"]["shape"]), "before lv_occ_configure", mode=sr.REPLACE, reach=1)
        ctx.occ_configure(_occ_params(capi, "coarse"))
        _call(capi, ctx, *vol, _unknown(sc.GRIDS["coarse"]["shape"]), "after lv_occ_configure", mode=sr.REPLACE, reach=1)


def test_end_to_end_without_a_lidar(capi):
    """depth images -> TSDF -> occupancy grid -> distance field (the ESDF of the surface) -> plan"""
    import depth_cases as dc
    import distance_ref as dr
    import occupancy_ref as ocr
    from limo_velo_amd import mesh

    with capi.Context() as ctx:
        ctx.tsdf_configure(capi.default_tsdf_params(origin=[float(v) for v in dc.ORIGIN], resolution=dc.RES, nx=dc.NX, ny=dc.NY, nz=dc.NZ,
                                                    trunc_cells=dc.TRUNC_CELLS))
        mesh.integrate_depth(ctx, dc.frames3(), capi.default_depth_params(min_depth=0.3, max_depth=5.0, carve=1))
        v = ctx.tsdf_fetch()
        S, W = v["S"], v["W"]
        st = mesh.to_occupancy(ctx, reach=1)   # no grid yet: one like the volume, then FILL
        op = ctx.occ_params()
        assert (op.nx, op.ny, op.nz, op.resolution) == (dc.NX, dc.NY, dc.NZ, F(dc.RES)) and list(op.origin) == list(ctx.tsdf_params().origin)
        grid, vg = _geometries(ctx)
        want, wst = sr.from_surface(_unknown(S.shape), grid, vg, S, W, reach=1, mode=sr.FILL)
        L = ctx.occ_fetch()
        assert np.array_equal(st, wst) and np.array_equal(L.view(np.uint32), want.view(np.uint32)) and st[0] > 1000 and st[1] > 5000 and st[3] == 0
        _, st = _call(capi, ctx, S, W, L, "REPLACE after to_occupancy", reach=1, mode=sr.REPLACE)
        assert st[2] == 0   # filled from nothing, the grid already was a pure function of the volume
        # the distance field of that grid equals the reference's on the reference's grid
        prm = ocr.params_of(op)
        ctx.occ_distance_build()
        s2, _ = ctx.occ_distance_fetch()
        rs2, _ = dr.build(prm, want, dr.dparams())
        assert np.array_equal(s2, rs2) and (want >= F(prm["l_occ"])).sum() == st[0]
        # a plan from one FREE voxel to another
        cls, _ = sr.classify(grid, vg, S, W, reach=1)
        k, j, i = np.nonzero(cls == sr.FREE)
        centre = lambda n: [float(sr.centres(grid["origin"][a], grid["resolution"], s)[c]) for a, (s, c) in enumerate(((dc.NX, i[n]), (dc.NY, j[n]), (dc.NZ, k[n])))]
        goal, start = len(k) // 3, 2 * len(k) // 3
        ctx.occ_plan_build(np.array([centre(goal)], F), np.array([50], np.uint8), capi.default_plan_params(connectivity=6))
        P, _ = ctx.occ_plan_fetch()
        print(f"plan: P = {P[k[start], j[start], i[start]]} at the start, {P[k[goal], j[goal], i[goal]]} at the goal")
        assert P[k[goal], j[goal], i[goal]] == 0 and 0 < P[k[start], j[start], i[start]] < 0xFFFFFFFF
