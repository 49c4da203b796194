"""lv_occ_raycast and lv_occ_view_gain (include/limovelo_hip.h "Ray casting") on the GPU, through capi, against tests/occ_ray_ref.py:
equality on every field, no tolerance.  The cases of tests/test_occ_ray_host.py on its 19 x 13 x 9 grid; a 70 x 37 x 11 grid built by
lv_occ_integrate (x rows end inside a 16-cell and a 32-cell word) with more rays than one workgroup and a ragged last wavefront;
a 1024 x 3 x 2 grid walked along x over every word; 32 views in one call; and what the calls must leave alone."""
import ctypes as C

import numpy as np
import pytest

import occ_ray_cases as cases
import occ_ray_ref as orr
import occupancy_ref as ocr

pytestmark = pytest.mark.gpu

LV_OK, LV_EINVAL, LV_ESTATE = 0, -1, -4
F = np.float32
PRM = cases.PRM
ID = np.eye(3, dtype=F)


@pytest.fixture(scope="module")
def capi(lv):
    from limo_velo_amd import capi as c

    return c


def _context(capi, prm, L=None):
    ctx = capi.Context()
    ctx.occ_configure(capi.default_occupancy_params(**prm))
    if L is not None:
        ctx.occ_load(L)
    return ctx


def _same(got, want):
    assert got.dtype == orr.RESULT_DTYPE
    for f in orr.RESULT_FIELDS:
        assert np.array_equal(got[f], want[f]), (f, np.nonzero(got[f] != want[f])[0][:8])


def _cast(capi, ctx, frm, to, su=False):
    return ctx.occ_raycast(frm, to, capi.default_ray_params(stop_unknown=int(su)))


def test_host_cases(capi):
    want = cases.ray_answers()
    with _context(capi, PRM, cases.grid()) as ctx:
        for (name, su), res in want.items():
            _same(_cast(capi, ctx, *cases.rays()[name], su), res)
        gains = cases.gain_answers()
        for name, (L, views) in cases.gain_views().items():
            ctx.occ_load(L)
            assert np.array_equal(ctx.occ_view_gain(views), gains[name]), name


@pytest.fixture(scope="module")
def built():
    """A 70 x 37 x 11 grid as three views leave it, and 32 views to look at it with."""
    prm = ocr.params(origin=(-3.0, -2.0, -0.5), resolution=0.1, nx=70, ny=37, nz=11, min_range=0.2, max_range=5.0)
    rng = np.random.default_rng(12)
    lo, hi = np.array(prm["origin"]), np.array(prm["origin"]) + np.array([70, 37, 11]) * 0.1

    def view(t, n, far):
        d = rng.normal(size=(n, 3))
        d /= np.linalg.norm(d, axis=1)[:, None]
        return cases._rot(rng), np.asarray(t, F), (d * rng.uniform(0.15, far, (n, 1))).astype(F)

    sweeps = [view((-1.0, -0.5, 0.0), 700, 3.0), view((2.5, 1.0, 0.3), 700, 3.0), view((0.3, -2.4, 0.1), 500, 6.0)]
    L, stats = ocr.integrate(prm, ocr.empty(prm), sweeps)
    frm = rng.uniform(lo - 0.4, hi + 0.4, (3000, 3)).astype(F)
    to = rng.uniform(lo - 0.4, hi + 0.4, (3000, 3)).astype(F)
    looks = [view(rng.uniform(lo - 0.2, hi + 0.2), 150, 6.0) for _ in range(32)]
    return dict(prm=prm, sweeps=sweeps, L=L, stats=stats, frm=frm, to=to, looks=looks, gain=orr.view_gain(prm, L, looks))


def test_integrated_grid_3000_rays_and_32_views(capi, built):
    prm, L = built["prm"], built["L"]
    with _context(capi, prm) as ctx:
        assert list(ctx.occ_integrate(built["sweeps"])) == list(built["stats"]) and ocr.same_bits(ctx.occ_fetch(), L)
        for su in (False, True):
            want = orr.raycast(prm, L, built["frm"], built["to"], su)
            _same(_cast(capi, ctx, built["frm"], built["to"], su), want)
            assert all((want["status"] == s).sum() > 100 for s in (orr.CLEAR, orr.STOPPED))
        gain = ctx.occ_view_gain(built["looks"])
        assert gain.shape == (32, 4) and np.array_equal(gain, built["gain"])
        assert np.all(gain[:, 0] > 0) and (gain[:, 1] > 0).sum() > 20 and (gain[:, 2] > 0).sum() > 20 and (gain[:, 3] > 0).sum() > 20
        # views are independent of their order, and of what shares the call with them
        assert np.array_equal(ctx.occ_view_gain(built["looks"][::-1]), built["gain"][::-1])
        assert np.array_equal(ctx.occ_view_gain(built["looks"][5:6]), built["gain"][5:6])
        # strided point arrays
        wide = np.zeros((3000, 2, 5), F)
        wide[:, 0, :3], wide[:, 1, 1:4] = built["frm"], built["to"]
        out = np.zeros(3000, capi.RAY_RESULT_DTYPE)
        p = capi.default_ray_params()
        assert ctx.lib.lv_occ_raycast(ctx.h, C.byref(p), wide.ctypes.data, 40, wide.ctypes.data + 24, 40, 3000,
                                      out.ctypes.data_as(C.POINTER(capi.RayResult))) == LV_OK
        _same(out, orr.raycast(prm, L, built["frm"], built["to"], False))


def test_long_rows_every_word(capi):
    prm = ocr.params(origin=(0.0, 0.0, 0.0), resolution=0.5, nx=1024, ny=3, nz=2, min_range=0.1, max_range=1000.0)
    y, z = np.meshgrid((0.25, 0.75, 1.25), (0.3, 0.8), indexing="ij")
    rows = np.stack([y.ravel(), z.ravel()], axis=1)
    left = np.hstack([np.full((6, 1), -0.4), rows])
    right = np.hstack([np.full((6, 1), 512.3), rows])
    frm = np.vstack([left, right, left, [[100.2, 0.25, 0.3]]]).astype(F)
    to = np.vstack([right, left, right + [0, 0.2, 0.1], [[7.9, 0.25, 0.3]]]).astype(F)   # +x, -x, a slant, and from inside
    with _context(capi, prm) as ctx:
        for i in (0, 15, 16, 31, 32, 1023):
            L = np.full((2, 3, 1024), -1.0, F)
            L[::2, ::2, 500:520] = np.nan
            L[:, :, i] = 1.0
            ctx.occ_load(L)
            wants = {su: orr.raycast(prm, L, frm, to, su) for su in (False, True)}
            for su, want in wants.items():
                _same(_cast(capi, ctx, frm, to, su), want)
            assert wants[True]["status"][0] == orr.STOPPED and wants[True]["cell"][0] == min(i, 500)
            want = wants[False]
            assert list(want["cell"][:6] % 1024) == [i] * 6 and list(want["steps"][:6]) == [i + 1] * 6
            assert list(want["cell"][6:12] % 1024) == [i] * 6 and list(want["steps"][6:12]) == [1024 - i] * 6


def test_cleared_grid_gain_is_what_integrate_updates(capi, built):
    """Code this change does not touch says the same: on a cleared grid every cell a view's rays stand in is unknown, and those
    are the cells lv_occ_integrate updates."""
    with _context(capi, built["prm"]) as ctx:
        gain = ctx.occ_view_gain(built["looks"])
        for v in (0, 7, 31):
            ctx.occ_clear()
            stats = ctx.occ_integrate(built["looks"][v:v + 1])
            assert gain[v][0] == stats[0] and gain[v][2] == stats[2] + stats[3] and gain[v][1] == 0 and gain[v][3] == 0
        assert (gain[:, 2] > 0).all()


def test_read_only_and_cache(capi, built):
    prm, L = built["prm"], built["L"]
    looks = built["looks"]
    with _context(capi, prm, L) as ctx:
        ctx.occ_distance_build(capi.default_distance_params())
        ctx.occ_plan_build(np.array([[0.0, 0.0, 0.0]], F), np.array([200, 90, 50], np.uint8), capi.default_plan_params(connectivity=26))
        ctx.occ_frontier_build(capi.default_frontier_params())
        s2, (P, pc), lab = ctx.occ_distance_fetch()[0], ctx.occ_plan_fetch(), ctx.occ_frontier_fetch()
        _cast(capi, ctx, built["frm"], built["to"])
        ctx.occ_view_gain(looks)
        assert ocr.same_bits(ctx.occ_fetch(), L)
        assert (ctx.occ_distance_info().stale, ctx.occ_plan_info().stale, ctx.occ_frontier_info().stale) == (0, 0, 0)
        P1, pc1 = ctx.occ_plan_fetch()
        assert np.array_equal(ctx.occ_distance_fetch()[0], s2) and np.array_equal(P1, P) and np.array_equal(pc1, pc)
        assert np.array_equal(ctx.occ_frontier_fetch(), lab)
        # the bitmaps were left all zero: an integrate issued after the gain gives the reference grid
        L2, stats = ocr.integrate(prm, L, looks[:2])
        assert list(ctx.occ_integrate(looks[:2])) == list(stats) and ocr.same_bits(ctx.occ_fetch(), L2)
        assert ctx.occ_distance_info().stale == 1
        # the live grid: the answers follow it
        _same(_cast(capi, ctx, built["frm"], built["to"]), orr.raycast(prm, L2, built["frm"], built["to"]))
        assert np.array_equal(ctx.occ_view_gain(looks), orr.view_gain(prm, L2, looks))
        ctx.occ_clear()
        res = _cast(capi, ctx, built["frm"], built["to"])
        assert not (res["status"] == orr.STOPPED).any() and (res["n_unknown"] > 0).any() and not res["n_free"].any()
    # a ray down a free corridor; then a view whose one return occupies a voxel on it
    prm = ocr.params(origin=(0.0, 0.0, 0.0), resolution=0.5, nx=40, ny=3, nz=3, min_range=0.1, max_range=30.0)
    L = np.full((3, 3, 40), prm["l_free"], F)   # (free, and one hit from occupied)
    frm, to = np.array([[0.25, 0.75, 0.75]], F), np.array([[19.75, 0.75, 0.75]], F)
    hit = (ID, np.array([10.25, 0.25, 0.75], F), np.array([[0.0, 0.5, 0.0]], F))   # ends in voxel (20, 1, 1)
    with _context(capi, prm, L) as ctx:
        a = _cast(capi, ctx, frm, to)
        ctx.occ_integrate([hit])
        b = _cast(capi, ctx, frm, to)
        La = ocr.integrate(prm, L, [hit])[0]
        _same(a, orr.raycast(prm, L, frm, to))
        _same(b, orr.raycast(prm, La, frm, to))
        assert a["status"][0] == orr.CLEAR and (b["status"][0], b["cell"][0], b["steps"][0]) == (orr.STOPPED, (1 * 3 + 1) * 40 + 20, 20)
        # reconfiguring frees the packed states: a grid of another shape is answered from its own
        prm2 = dict(prm, nx=33, ny=5)
        ctx.occ_configure(capi.default_occupancy_params(**prm2))
        L3 = np.full((3, 5, 33), -1.0, F)
        L3[1, 1, 17] = 1.0
        ctx.occ_load(L3)
        _same(_cast(capi, ctx, frm, to), orr.raycast(prm2, L3, frm, to))


def test_state_and_empty_calls(capi):
    with capi.Context() as ctx:
        p = capi.default_ray_params()
        pts = np.ones((2, 3), F)
        out = np.full(2, 9, np.uint8).repeat(32).view(capi.RAY_RESULT_DTYPE)
        gain = (C.c_uint64 * 4)(7, 7, 7, 7)
        arr, keep = capi.view_array([(ID, np.zeros(3, F), pts)])
        args = (C.byref(p), pts.ctypes.data, 12, pts.ctypes.data, 12)
        assert ctx.lib.lv_occ_raycast(ctx.h, *args, 2, out.ctypes.data_as(C.POINTER(capi.RayResult))) == LV_ESTATE
        assert ctx.lib.lv_occ_raycast(ctx.h, *args, 0, None) == LV_ESTATE
        assert ctx.lib.lv_occ_view_gain(ctx.h, arr, 1, gain) == LV_ESTATE
        assert np.all(out.view(np.uint8) == 9) and list(gain) == [7] * 4
        ctx.occ_configure(capi.default_occupancy_params(**PRM))
        assert ctx.lib.lv_occ_raycast(ctx.h, *args, 0, out.ctypes.data_as(C.POINTER(capi.RayResult))) == LV_OK
        assert ctx.lib.lv_occ_raycast(ctx.h, C.byref(p), None, 0, None, 0, 0, None) == LV_OK
        assert np.all(out.view(np.uint8) == 9)
        assert len(ctx.occ_raycast(np.zeros((0, 3), F), np.zeros((0, 3), F))) == 0
        assert ctx.lib.lv_occ_raycast(ctx.h, None, pts.ctypes.data, 12, pts.ctypes.data, 12, 2, out.ctypes.data_as(C.POINTER(capi.RayResult))) == LV_EINVAL
        assert ctx.lib.lv_occ_view_gain(ctx.h, arr, 33, gain) == LV_EINVAL and np.all(out.view(np.uint8) == 9) and list(gain) == [7] * 4
        assert ctx.lib.lv_occ_view_gain(ctx.h, arr, 1, gain) == LV_OK and list(gain)[1:] == [0, list(gain)[2], 0] and gain[2] > 0


def test_simulate_scan_and_line_of_sight(capi):
    from limo_velo_amd import occupancy

    L = cases.grid()
    with _context(capi, PRM, L) as ctx:
        pattern = occupancy.scan_pattern(36, 5, -0.4, 0.4, 3.0)
        assert pattern.shape == (180, 3) and pattern.dtype == F and np.allclose(np.linalg.norm(pattern, axis=1), 3.0)
        rng = np.random.default_rng(4)
        R, t = cases._rot(rng), np.array([0.1, 0.2, 0.3], F)
        got = occupancy.simulate_scan(ctx, R, t, pattern)
        to = (pattern @ R.T + t).astype(F)
        frm = np.tile(t, (len(to), 1))
        res = orr.raycast(PRM, L, frm, to)
        want = orr.range_m(PRM, frm, to, res)
        assert got.dtype == np.float64 and np.array_equal(got, want)
        assert np.isinf(want).any() and np.isfinite(want).any() and np.all(want[np.isfinite(want)] <= 3.01)
        res2, rng_m = occupancy.raycast(ctx, *cases.rays()["ignored"], stop_unknown=True)
        _same(res2, cases.ray_answers()[("ignored", True)])
        assert np.all(np.isnan(rng_m[:8])) and not np.isnan(rng_m[8])
        frm, to = cases.rays()["random0"]
        assert np.array_equal(occupancy.line_of_sight(ctx, frm, to), cases.ray_answers()[("random0", False)]["status"] == orr.CLEAR)


def test_explore_with_and_without_gain(capi):
    """The two rooms of tests/test_gpu_occ_frontier.py: without gain_pattern explore() is what it was, field for field; with one
    the clusters also carry view_gain at their targets."""
    from limo_velo_amd import occupancy

    prm = ocr.params(origin=(0.0, 0.0, 0.0), resolution=0.25, nx=40, ny=16, nz=1)
    L = np.full((1, 16, 40), prm["l_max"], F)
    L[0, 1:15, 1:19] = prm["l_min"]
    L[0, 1:15, 21:39] = prm["l_min"]
    L[0, 7:9, 19:21] = prm["l_min"]
    L[0, 15, 5:8] = np.nan
    L[0, 0, 30:33] = np.nan
    robot = np.array([10.5 * 0.25, 7.5 * 0.25, 0.1], F)
    with _context(capi, prm, L) as ctx:
        found, lines = occupancy.explore(ctx, robot, 0.1, z_band=(0.0, 0.25))
        assert found.dtype.names == capi.FRONTIER_CLUSTER_DTYPE.names + ("rep_xyz", "centre_xyz", "label", "best_p", "best_cell", "target_xyz")
        assert len(found) == 2 and list(found["label"]) == [1, 0] and found["best_p"][0] < found["best_p"][1] < capi.LV_PLAN_UNREACHED
        assert found["target_xyz"][0][0] < 19 * 0.25 < found["target_xyz"][1][0]
        for c in range(2):
            assert np.allclose(lines[c][0], robot[:2]) and np.allclose(lines[c][-1], found["target_xyz"][c][:2])
        pattern = occupancy.scan_pattern(90, 1, 0.0, 0.0, 3.0)
        with_gain, lines2 = occupancy.explore(ctx, robot, 0.1, z_band=(0.0, 0.25), gain_pattern=pattern)
        assert with_gain.dtype.names == found.dtype.names + ("gain_unknown", "gain_free")
        for f in found.dtype.names:
            assert np.array_equal(with_gain[f], found[f]), f
        assert all(np.array_equal(a, b) for a, b in zip(lines, lines2))
        gain = occupancy.view_gain(ctx, found["target_xyz"], pattern)
        views = [(ID, t, pattern) for t in found["target_xyz"]]
        assert np.array_equal(gain, orr.view_gain(prm, L, views))
        assert np.array_equal(with_gain["gain_unknown"], gain[:, 2]) and np.array_equal(with_gain["gain_free"], gain[:, 3])
        assert np.all(gain[:, 2] > 0) and np.all(gain[:, 1] > 0)
        assert occupancy.view_gain(ctx, found["target_xyz"], pattern, yaws=[0.3, -1.2]).shape == (2, 4)
        # 33 positions: two calls
        many = occupancy.view_gain(ctx, np.tile(found["target_xyz"][:1], (33, 1)), pattern)
        assert many.shape == (33, 4) and np.all(many == gain[0])
