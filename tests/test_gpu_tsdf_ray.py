"""GPU tests of the ray casting on the TSDF surface (lv_tsdf_ray.hip; include/limovelo_hip.h "Surface ray casting") against the
numpy statement of the rule in tests/tsdf_ray_ref.py, on the shared cases of tests/tsdf_ray_cases.py.  Everything is held by
equality: every field of every record, every bit of every normal, every byte of every colour."""
import numpy as np
import pytest

import colour_ref as cr
import tsdf_cases as tc
import tsdf_ray_cases as cases
import tsdf_ray_ref as trr

pytestmark = pytest.mark.gpu

F = np.float32


@pytest.fixture(scope="module")
def capi(lv):
    from limo_velo_amd import capi as c

    return c


def _configure(capi, ctx, prm):
    ctx.tsdf_configure(capi.default_tsdf_params(origin=[float(v) for v in prm["origin"]], **{k: prm[k] for k in tc.tr.FIELDS if k != "origin"}))


def _build(capi, ctx, c, load=False):
    """The case's volume on the device: by its lv_tsdf_integrate calls (and its recentre), or by lv_tsdf_load."""
    if load or "source" not in c:
        _configure(capi, ctx, c["prm"])
        ctx.tsdf_load(c["S"], c["W"])
    else:
        _configure(capi, ctx, c["source"]["prm"])
        for views in c["source"]["calls"]:
            ctx.tsdf_integrate(views)
        if "shift" in c:
            ctx.volume_recentre(capi.LV_VOLUME_SURFACE, c["shift"])
    vol = ctx.tsdf_fetch()
    assert np.array_equal(vol["S"], c["S"]) and np.array_equal(vol["W"], c["W"])
    assert trr.ocr.same_bits(np.array(list(ctx.tsdf_params().origin), F), np.asarray(c["prm"]["origin"], F))


def _same(got, want, what):
    for f in trr.RESULT_FIELDS:
        assert np.array_equal(got[0][f], want[0][f]), (what, f, np.nonzero(got[0][f] != want[0][f])[0][:8])
    if got[1] is not None:
        assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32)), (what, "normals")
    if got[2] is not None:
        assert np.array_equal(got[2], want[2]), (what, "rgba")


def _cast(capi, ctx, frm, to, mw=1, normals=True, colours=True):
    return ctx.tsdf_raycast(frm, to, capi.default_tsdf_ray_params(min_weight=mw), normals, colours)


@pytest.mark.parametrize("name", [c["name"] for c in cases.cases()])
def test_rays_of_every_case(capi, name):
    c = cases.case(name)
    frm, to, _ = cases.all_rays(c)
    mws = c["min_weights"]
    with capi.Context() as ctx:
        _build(capi, ctx, c)
        # no layer yet: colours are zeros, and asking for them allocates none
        got = _cast(capi, ctx, frm, to, mws[0])
        _same(got, cases.all_answers(c, mws[0], coloured=False), (name, "no layer"))
        assert not got[2].any() and ctx.colour_info().present == 0
        ctx.colour_load(c["layer"])
        for mw in mws:
            _same(_cast(capi, ctx, frm, to, mw), cases.all_answers(c, mw), (name, mw))
        bare = _cast(capi, ctx, frm, to, mws[0], False, False)
        assert bare[1] is None and bare[2] is None
        _same(bare, cases.all_answers(c, mws[0]), (name, "records only"))
        _same(_cast(capi, ctx, frm, to, mws[0], True, False), cases.all_answers(c, mws[0]), (name, "normals only"))
        _same(_cast(capi, ctx, frm, to, mws[0], False, True), cases.all_answers(c, mws[0]), (name, "colours only"))
        assert len(ctx.tsdf_raycast(np.zeros((0, 3), F), np.zeros((0, 3), F))[0]) == 0     # n = 0 succeeds
        if "source" in c:   # the same volume and layer by lv_tsdf_load: the same answers
            _build(capi, ctx, c, load=True)
            ctx.colour_load(c["layer"])
            _same(_cast(capi, ctx, frm, to, mws[0]), cases.all_answers(c, mws[0]), (name, "loaded"))


def _views():
    rng = np.random.default_rng(11)
    return [tc.random_view(rng, tc.INSIDE, 600), tc.random_view(rng, tc.OUTSIDE, 600), (tc.ID, np.array([np.nan, 0, 0], F), np.ones((5, 3), F)),
            (tc.ID, np.asarray(tc.INSIDE, F), np.zeros((0, 3), F)), tc.wall_view(tc.INSIDE, 200)]


def _implied(prm, R, t, pts):
    """The world end points of one view's returns as lv_tsdf_integrate forms them (f32, unfused): cut to max_range, then R p + t."""
    pts, R, t = np.asarray(pts, F).reshape(-1, 3), np.asarray(R, F).reshape(3, 3), np.asarray(t, F)
    x, y, z = pts[:, 0], pts[:, 1], pts[:, 2]
    with np.errstate(all="ignore"):
        r2 = x * x + y * y + z * z
        mx = F(prm["max_range"])
        cut = r2 > mx * mx
        s = np.where(cut, mx / np.sqrt(r2), F(1)).astype(F)
        x, y, z = (np.where(cut, v * s, v).astype(F) for v in (x, y, z))
        return np.stack([((R[a, 0] * x + R[a, 1] * y) + R[a, 2] * z) + t[a] for a in range(3)], axis=1).astype(F)


def test_views_are_the_rays_they_imply(capi):
    c = cases.case("33x17x9-carve1-3views")
    prm, views = c["prm"], _views()
    want = trr.raycast_views(prm, c["S"], c["W"], views, 1, c["layer"])
    with capi.Context() as ctx:
        _build(capi, ctx, c)
        ctx.colour_load(c["layer"])
        got = ctx.tsdf_raycast_views(views, None, True, True)
        _same(got, want, "views")
        assert np.array_equal(got[3], want[3]), (got[3], want[3])
        bare = ctx.tsdf_raycast_views(views)
        assert bare[1] is None and bare[2] is None and np.array_equal(bare[3], want[3])
        _same(bare, want, "views, records only")
        at = 0
        for R, t, pts in views:
            n = len(np.asarray(pts).reshape(-1, 3))
            part = tuple(a[at:at + n] for a in got[:3])
            at += n
            if n == 0 or not np.all(np.isfinite(t)):
                assert np.all(part[0]["status"] == trr.IGNORED)
                continue
            used, _ = trr.used_returns(prm, R, t, pts)
            assert np.array_equal(part[0]["status"] != trr.IGNORED, used)
            rays = _cast(capi, ctx, np.tile(np.asarray(t, F), (int(used.sum()), 1)), _implied(prm, R, t, pts)[used])
            _same(tuple(a[used] for a in part), rays, "the rays of a view")
    st = want[3]
    assert st[0] == st[1] + st[2] + st[3] and st[0] > 500 and np.all(st[1:] > 0) and st[0] < len(want[0])


def _few(c, n=3):
    """The first n random ray sets of a case in one pair of arrays."""
    names = [f"random{p}" for p in range(n)]
    return np.concatenate([c["rays"][k][0] for k in names]), np.concatenate([c["rays"][k][1] for k in names])


def test_the_packed_copy_follows_the_volume(capi):
    a, d = cases.case(cases.SOURCES[0]), cases.case("dense-21x4x3")
    frm, to = _few(a)
    prm, calls = a["prm"], a["source"]["calls"]
    with capi.Context() as ctx:
        _configure(capi, ctx, prm)
        S0, W0 = tc.tr.empty(prm)
        seen = []
        S, W = S0, W0
        for views in calls:                                            # lv_tsdf_integrate, call by call
            ctx.tsdf_integrate(views)
            S, W, _ = tc.tr.integrate(prm, S, W, views)
            want = trr.raycast(prm, S, W, frm, to)
            _same(_cast(capi, ctx, frm, to), want, "after integrate")
            seen.append(want[0])
        assert not np.array_equal(seen[0], seen[1])
        one, two = trr.raycast(prm, S, W, frm, to, 1), trr.raycast(prm, S, W, frm, to, 2)   # min_weight between calls, there and back
        assert not np.array_equal(one[0], two[0])
        _same(_cast(capi, ctx, frm, to, 2), two, "min_weight 2")
        _same(_cast(capi, ctx, frm, to, 1), one, "min_weight 1 again")
        ctx.volume_recentre(capi.LV_VOLUME_SURFACE, cases.SHIFT)       # a recentre
        moved = dict(prm, origin=cases.shifted_origin(prm["origin"], prm["resolution"], cases.SHIFT))
        Sm, Wm = cr.shift_layer(S, cases.SHIFT), cr.shift_layer(W, cases.SHIFT)
        want = trr.raycast(moved, Sm, Wm, frm, to)
        assert not np.array_equal(want[0], one[0])
        _same(_cast(capi, ctx, frm, to), want, "after recentre")
        S2 = np.where(Wm > 0, -np.abs(Sm) // 2, 0).astype(np.int32)     # lv_tsdf_load: everything observed is inside
        ctx.tsdf_load(S2, Wm)
        want = trr.raycast(moved, S2, Wm, frm, to)
        assert (want[0]["status"] == trr.BLOCKED).any() and not (want[0]["status"] == trr.HIT).any()
        _same(_cast(capi, ctx, frm, to), want, "after load")
        ctx.tsdf_clear()                                               # lv_tsdf_clear: nothing known, nothing stops a ray
        got = _cast(capi, ctx, frm, to)
        _same(got, trr.raycast(moved, S0, W0, frm, to), "after clear")
        assert np.all(got[0]["status"] == trr.CLEAR) and not got[0]["n_known"].any() and got[0]["n_unknown"].any()
        _configure(capi, ctx, d["prm"])                                # a reconfigure: another box, another packed size
        fd, td = _few(d)
        got = _cast(capi, ctx, fd, td)
        assert np.all(got[0]["status"] == trr.CLEAR)
        ctx.tsdf_load(d["S"], d["W"])
        _same(_cast(capi, ctx, fd, td, 2), trr.raycast(d["prm"], d["S"], d["W"], fd, td, 2), "after reconfigure")


def test_the_calls_change_nothing(capi):
    c = cases.case("sphere-6")
    frm, to = _few(c)
    case = c["source"]
    view = case["calls"][0][0]
    with capi.Context() as ctx:
        _build(capi, ctx, c)
        ctx.colour_load(c["layer"])
        ctx.tsdf_mesh_build(1)

        def snapshot():
            info = ctx.tsdf_mesh_info()
            return (ctx.tsdf_fetch(), ctx.colour_fetch()["sums"], ctx.tsdf_mesh_fetch(), ctx.mesh_colours(),
                    (info.built, info.stale, info.vertices, info.triangles), tuple(ctx.volume_shift_info().surface))

        def unchanged(a, b):
            assert all(np.array_equal(a[0][k], b[0][k]) for k in a[0]) and np.array_equal(a[1], b[1])
            assert all(np.array_equal(a[2][k], b[2][k]) for k in a[2]) and np.array_equal(a[3], b[3]) and a[4:] == b[4:]

        before = snapshot()
        assert before[4][:2] == (1, 0)
        _cast(capi, ctx, frm, to)
        _cast(capi, ctx, frm, to, 2, False, False)
        ctx.tsdf_raycast_views([view], None, True, True)
        unchanged(before, snapshot())
        ctx.colour_clear()                                             # a stale mesh stays stale, and the cleared layer gives no colour
        stale = snapshot()
        assert stale[4][:2] == (1, 1)
        got = _cast(capi, ctx, frm, to)
        assert not got[2].any() and (got[0]["status"] == trr.HIT).any()
        unchanged(stale, snapshot())


def test_simulate_scan_and_render_on_the_sphere(capi):
    from limo_velo_amd import mesh, occupancy

    c = cases.case("sphere-6")
    prm, S, W, layer = c["prm"], c["S"], c["W"], c["layer"]
    case = c["source"]
    centre = (np.asarray(prm["origin"], np.float64) + case["centre"] * prm["resolution"])
    with capi.Context() as ctx:
        _build(capi, ctx, c)
        ctx.colour_load(layer)
        # a scan from beside the centre, turned
        R = tc.rot(np.random.default_rng(3))
        t = (centre + (0.4, -0.3, 0.2)).astype(F)
        pattern = occupancy.scan_pattern(48, 12, -0.9, 0.9, 0.45)      # (0.45 m: below min_range, every return ignored)
        rng, pts = mesh.simulate_scan(ctx, R, t, pattern)
        assert np.all(np.isnan(rng)) and np.all(np.isnan(pts))
        pattern = occupancy.scan_pattern(48, 12, -0.9, 0.9, 8.0)
        rng, pts = mesh.simulate_scan(ctx, R, t, pattern)
        res, _, _, _ = trr.raycast_views(prm, S, W, [(R, t, pattern)], 1, layer)
        want = trr.metres(prm, res)
        want[res["status"] == trr.BLOCKED] = np.inf
        assert np.array_equal(rng, want, equal_nan=True) and rng.dtype == F
        assert (res["status"] == trr.HIT).sum() > 500
        unit = pattern.astype(np.float64) / np.linalg.norm(pattern.astype(np.float64), axis=1)[:, None]
        hit = np.isfinite(want)
        assert np.allclose(pts[hit], unit[hit] * want[hit].astype(np.float64)[:, None], rtol=1e-12, atol=0) and np.all(np.isnan(pts[~hit]))
        world = pts[hit] @ R.astype(np.float64).T + t                  # the hit points lie on the sphere (3 m) to a fraction of a voxel
        assert np.abs(np.linalg.norm(world - centre, axis=1) - case["radius"] * prm["resolution"]).max() < 0.25 * prm["resolution"]
        # a camera at the centre looking along world +x: camera x = world -y, camera y = world -z, camera z = world x
        Rc = np.array([[0, 0, 1], [-1, 0, 0], [0, -1, 0]], F)
        tc_ = centre.astype(F)
        w, h, fx, fy, cx, cy = 64, 48, 40.0, 42.0, 31.5, 23.5
        depth, nrm, rgba = mesh.render(ctx, Rc, tc_, fx, fy, cx, cy, w, h, max_range=6.0)
        assert depth.shape == (h, w) and nrm.shape == (h, w, 3) and rgba.shape == (h, w, 4) and depth.dtype == F and rgba.dtype == np.uint8
        v, u = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
        d = np.stack([(u - cx) / fx, (v - cy) / fy, np.ones_like(u)], axis=-1).reshape(-1, 3)
        d /= np.linalg.norm(d, axis=1)[:, None]
        ends = (6.0 * d).astype(F)
        assert np.array_equal(mesh.camera_pattern(fx, fy, cx, cy, w, h, 6.0), ends)
        res, wn, wc, _ = trr.raycast_views(prm, S, W, [(Rc, tc_, ends)], 1, layer)
        assert np.all(res["status"] == trr.HIT)
        unit = ends.astype(np.float64) / np.linalg.norm(ends.astype(np.float64), axis=1)[:, None]
        zd = (trr.metres(prm, res).astype(np.float64) * unit[:, 2]).astype(F)
        assert np.array_equal(depth.reshape(-1), zd)
        assert np.array_equal(nrm.reshape(-1, 3).view(np.uint32), wn.view(np.uint32)) and np.array_equal(rgba.reshape(-1, 4), wc) and wc.any()
        # the depth image is the sphere's: z = 3 m times the ray's z component, to a fraction of a voxel
        assert np.abs(depth.reshape(-1) - 3.0 * unit[:, 2]).max() < 0.25 * prm["resolution"]
        # a camera outside looking away sees nothing: NaN depth, zero normals and colours
        depth, nrm, rgba = mesh.render(ctx, Rc, (centre + (5.0, 0, 0)).astype(F), fx, fy, cx, cy, 16, 12, max_range=3.0)
        assert np.all(np.isnan(depth)) and not nrm.any() and not rgba.any()
