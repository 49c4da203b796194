"""GPU tests of the colour layer (lv_colour.hip; include/limovelo_hip.h "Colour layer") against the numpy statement of the rule in
tests/colour_ref.py.  The volume comes from lv_tsdf_load (tests/colour_cases.py: a wall and a floor, three cameras).  The layer
must equal the reference on every decided voxel (see paint_ref.py) and lie inside its interval on the others, whose share is held
below 1 % of the possible (voxel, view) decisions: a condition on the scene, not a tolerance."""
import ctypes as C

import numpy as np
import pytest

import colour_cases as cc
import colour_ref as cr

pytestmark = pytest.mark.gpu

LV_EINVAL, LV_ESTATE = -1, -4
CAP = 0.01


@pytest.fixture(scope="module")
def capi(lv):
    from limo_velo_amd import capi as c

    return c


@pytest.fixture(scope="module")
def vol():
    S, W = cc.volume()
    S.setflags(write=False)
    W.setflags(write=False)
    return S, W


def _open(capi, S, W, origin=cc.ORIGIN):
    ctx = capi.Context()
    nz, ny, nx = S.shape
    ctx.tsdf_configure(capi.default_tsdf_params(origin=[float(v) for v in origin], resolution=cc.RES, nx=nx, ny=ny, nz=nz,
                                                trunc_cells=cc.TRUNC_CELLS))
    ctx.tsdf_load(S, W)
    return ctx


def _params(capi, zbuf_scale=16, window=1, **kw):
    kw.setdefault("min_weight", 2)
    return capi.default_colour_params(zbuf_scale=zbuf_scale, window=window, margin_abs=0.5, **kw)


def _check(got, stats, ref, before, what, min_coloured=1000, max_weight=64):
    """The fetched layer and the stats of one call against the reference of that call (before: the layer it started from)."""
    g, want, b = got.reshape(-1, 4), ref["after"].reshape(-1, 4), before.reshape(-1, 4)
    flat, dec = ref["flat"], ref["decided"]
    share = ref["undecided"] / max(ref["possible"], 1)
    print(f"{what}: {len(flat)} candidates, {ref['possible']} possible decisions, {ref['undecided']} undecided ({100 * share:.3f} %), "
          f"stats {stats} in {ref['stats_lo']}..{ref['stats_hi']}, {int((g[:, 3] > 0).sum())} coloured")
    assert share < CAP, share
    d = flat[dec]
    bad = np.flatnonzero((g[d] != want[d]).any(axis=1))
    assert bad.size == 0, f"{what}: {bad.size} decided voxels differ, first {d[bad[:4]]}: got {g[d[bad[:4]]]} want {want[d[bad[:4]]]}"
    rest = np.ones(len(g), bool)
    rest[flat] = False
    assert np.array_equal(g[rest], b[rest]), f"{what}: a voxel that is no candidate changed"
    u, lo, hi = flat[~dec], ref["lo"][~dec], ref["hi"][~dec]
    w0, w1 = b[u, 3].astype(np.int64), g[u, 3].astype(np.int64)   # an undecided voxel: Wc counts the seeing views, up to the cap
    assert np.all((w1 >= np.minimum(w0 + lo, max_weight)) & (w1 <= np.minimum(w0 + hi, max_weight))), f"{what}: an undecided voxel outside its interval"
    assert int(stats[0]) == int(ref["stats_lo"][0])
    assert np.all(stats[1:] >= ref["stats_lo"][1:]) and np.all(stats[1:] <= ref["stats_hi"][1:]), (stats, ref["stats_lo"], ref["stats_hi"])
    assert (g[:, 3] > 0).sum() > min_coloured


@pytest.mark.parametrize("scale,window,width,height,focal", cc.SETTINGS)
def test_parity_flat_images(capi, vol, scale, window, width, height, focal):
    S, W = vol
    frames = cc.frames(width, height, focal)
    prm = _params(capi, scale, window)
    with _open(capi, S, W) as ctx:
        assert ctx.colour_info().present == 0
        stats = ctx.colour_integrate(frames, prm)
        got = ctx.colour_fetch()["sums"]
        info = ctx.colour_info()
    ref = cr.integrate(S, W, None, cc.ORIGIN, cc.RES, frames, prm)
    _check(got, stats, ref, np.zeros_like(got), f"flat {scale} x {window} at {width} x {height}")
    assert info.present == 1 and info.voxels == S.size and info.coloured == (got[..., 3] > 0).sum()
    assert np.all(got[..., :3] <= 255 * got[..., 3:4])


def test_smooth_images_within_one_level(capi, vol):
    from test_gpu_map_paint import smooth_image

    S, W = vol
    images = [smooth_image(640, 480, 1), smooth_image(640, 480, 2), smooth_image(640, 480, 3, channels=1)]
    frames = cc.frames(images=images)
    prm = _params(capi)
    with _open(capi, S, W) as ctx:
        ctx.colour_integrate(frames, prm)
        out = ctx.colour_fetch(sums=True, rgba=True)
    ref = cr.integrate(S, W, None, cc.ORIGIN, cc.RES, frames, prm)
    d = ref["flat"][ref["decided"] & (ref["lo"] > 0)]
    got = out["rgba"].reshape(-1, 4)[d].astype(np.int64)
    want = cr.voxel_colour(ref["after"].reshape(-1, 4)[d]).astype(np.int64)
    err = np.abs(got - want).max()
    print(f"smooth: max |colour - ref| {err} levels over {len(d)} voxels, {int((got != want).any(axis=1).sum())} differ")
    assert len(d) > 1000 and err <= 1
    assert np.array_equal(out["rgba"], cr.voxel_colour(out["sums"]))   # (the voxel colour of the fetched sums, exactly)
    assert np.array_equal(out["sums"].reshape(-1, 4)[d, 3], ref["lo"][ref["decided"] & (ref["lo"] > 0)])


def test_fold_recurrence_and_view_order(capi, vol):
    S, W = vol
    frames = cc.frames()
    prm = _params(capi, max_weight=3)
    layer = np.zeros(S.shape + (4,), np.uint32)
    with _open(capi, S, W) as ctx, _open(capi, S, W) as other:
        for call in range(5):
            stats = ctx.colour_integrate(frames, prm)
            other.colour_integrate([frames[2], frames[0], frames[1]], prm)
            got = ctx.colour_fetch()["sums"]
            ref = cr.integrate(S, W, layer, cc.ORIGIN, cc.RES, frames, prm)
            _check(got, stats, ref, layer, f"fold, call {call}", max_weight=3)
            layer = got
        assert got[..., 3].max() == 3 and np.all(got[..., :3] <= 255 * got[..., 3:4])
        assert np.array_equal(other.colour_fetch()["sums"], got)   # the views permuted: bit-equal over every voxel


def _painted_mesh(capi, S, W, frames, prm):
    with _open(capi, S, W) as ctx:
        ctx.colour_integrate(frames, prm)
        ctx.colour_integrate(frames[:2], prm)
        counts = ctx.tsdf_mesh_build(1)
        return ctx.colour_fetch()["sums"], ctx.mesh_colours(), counts, ctx.tsdf_mesh_info().reserved


def test_determinism_and_vertex_colours(capi, vol):
    S, W = vol
    frames = cc.frames()
    prm = _params(capi)
    layer, rgba, counts, reserved = _painted_mesh(capi, S, W, frames, prm)
    layer2, rgba2, _, _ = _painted_mesh(capi, S, W, frames, prm)
    assert np.array_equal(layer, layer2) and np.array_equal(rgba, rgba2)
    want = cr.mesh_colours(S, W, layer, 1)
    assert reserved == 1 and len(rgba) == int(counts[0]) == len(want) > 1000
    assert np.array_equal(rgba, want)
    k = (rgba[:, 3] == 255).sum()
    print(f"vertex colours: {len(rgba)} vertices, {int(k)} coloured")
    assert 100 < k < len(rgba)   # both branches of the rule
    with _open(capi, S, W) as ctx:   # a mesh built before any colour call carries none
        ctx.tsdf_mesh_build(1)
        assert ctx.tsdf_mesh_info().reserved == 0 and ctx.colour_info().present == 0
        buf = np.zeros((int(counts[0]), 4), np.uint8)
        assert ctx.lib.lv_mesh_colours(ctx.h, buf.ctypes.data_as(C.POINTER(C.c_uint8)), len(buf)) == LV_ESTATE
        ctx.colour_integrate(frames, prm)   # ... and goes on carrying none until it is built again
        assert ctx.tsdf_mesh_info().stale == 1
        assert ctx.lib.lv_mesh_colours(ctx.h, buf.ctypes.data_as(C.POINTER(C.c_uint8)), len(buf)) == LV_ESTATE
        ctx.tsdf_mesh_build(1)
        assert ctx.tsdf_mesh_info().reserved == 1 and np.array_equal(ctx.mesh_colours(), cr.mesh_colours(S, W, ctx.colour_fetch()["sums"], 1))


def test_rolling_moves_the_layer(capi, vol):
    S, W = vol
    frames = cc.frames()
    prm = _params(capi)
    d = (3, -2, 1)
    with _open(capi, S, W) as ctx:
        ctx.colour_integrate(frames, prm)
        L = ctx.colour_fetch()["sums"]
        ctx.volume_recentre(capi.LV_VOLUME_SURFACE, (0, 0, 0))
        assert np.array_equal(ctx.colour_fetch()["sums"], L)
        ctx.volume_recentre(capi.LV_VOLUME_SURFACE, d)
        moved = ctx.colour_fetch()["sums"]
        assert np.array_equal(moved, cr.shift_layer(L, d)) and (moved[..., 3] > 0).sum() > 1000
        v = ctx.tsdf_fetch()
        assert np.array_equal(v["S"], cr.shift_layer(S, d)) and np.array_equal(v["W"], cr.shift_layer(W, d))
        origin = [float(x) for x in ctx.tsdf_params().origin]
        stats = ctx.colour_integrate(frames, prm)   # a paint at the new origin
        ref = cr.integrate(v["S"], v["W"], moved, origin, cc.RES, frames, prm)
        after = ctx.colour_fetch()["sums"]
        _check(after, stats, ref, moved, "after the shift")
        ctx.volume_recentre(capi.LV_VOLUME_SURFACE, [-x for x in d])
        assert np.array_equal(ctx.colour_fetch()["sums"], cr.shift_layer(after, [-x for x in d]))   # survivors bit-equal, the rest zero
        ctx.volume_recentre(capi.LV_VOLUME_SURFACE, (0, 0, -64))   # everything leaves
        assert not ctx.colour_fetch()["sums"].any() and ctx.colour_info().present == 1


ODD_ORIGIN = (-1.0, -2.9, -2.0)


@pytest.mark.parametrize("case", ["odd", "band", "one", "many"])
def test_shapes(capi, vol, case):
    S, W = cc.volume(37, 29, 11, ODD_ORIGIN) if case == "odd" else vol   # 37 x 29 x 11: tails in every pass
    origin = ODD_ORIGIN if case == "odd" else cc.ORIGIN
    frames = cc.frames(n={"one": 1, "many": 32}.get(case, 3))
    prm = _params(capi, band=cc.T if case == "band" else 256)
    with _open(capi, S, W, origin) as ctx:
        stats = ctx.colour_integrate(frames, prm)
        got = ctx.colour_fetch()["sums"]
        if case == "odd":
            ctx.volume_recentre(capi.LV_VOLUME_SURFACE, (-1, 2, 0))
            assert np.array_equal(ctx.colour_fetch()["sums"], cr.shift_layer(got, (-1, 2, 0)))
            pts = cr.centres(ctx.tsdf_params().origin, cc.RES, S.shape, np.arange(S.size))
            assert np.array_equal(ctx.colour_query(pts), ctx.colour_fetch(sums=False, rgba=True)["rgba"].reshape(-1, 4))
            assert not ctx.colour_query(np.array([[1e3, 0, 0], [np.nan, 0, 0]], np.float32)).any()
    ref = cr.integrate(S, W, None, origin, cc.RES, frames, prm)
    _check(got, stats, ref, np.zeros_like(got), case, min_coloured={"odd": 300, "band": 500}.get(case, 1000))   # (band = T: every known voxel is a candidate and occludes)
    if case == "many":
        assert got[..., 3].max() > 16


def test_no_candidates(capi, vol):
    S, W = vol
    with _open(capi, np.zeros_like(S), np.zeros_like(W)) as ctx:
        stats = ctx.colour_integrate(cc.frames(), _params(capi))
        assert not stats.any() and ctx.colour_info().present == 1 and ctx.colour_info().coloured == 0
        assert not ctx.colour_fetch()["sums"].any()


def test_states_and_stale_rows(capi, vol):
    S, W = vol
    frames = cc.frames()
    prm = _params(capi)
    sweep = [(np.eye(3, dtype=np.float32), np.zeros(3, np.float32), np.array([[2.0, 0.1, 0.2]], np.float32))]
    with capi.Context() as ctx:   # before lv_tsdf_configure: LV_ESTATE from every call
        for call in (lambda: ctx.colour_integrate(frames, prm), ctx.colour_fetch, ctx.colour_clear, ctx.colour_info, ctx.mesh_colours,
                     lambda: ctx.colour_load(np.zeros(4, np.uint32)), lambda: ctx.colour_query(np.zeros((1, 3), np.float32))):
            with pytest.raises(capi.LvError, match="error -4: no TSDF volume"):
                call()
    with _open(capi, S, W) as ctx:
        ctx.tsdf_integrate(sweep)
        ctx.tsdf_mesh_build(1)
        assert ctx.colour_info().present == 0   # an integrate and a mesh build allocate no layer
        for call in (ctx.colour_fetch, lambda: ctx.colour_query(np.zeros((1, 3), np.float32))):
            with pytest.raises(capi.LvError, match="error -4: no colour layer"):
                call()
        ctx.colour_clear()   # LV_OK, nothing done
        assert ctx.colour_info().present == 0 and ctx.tsdf_mesh_info().stale == 0
        ctx.colour_integrate(frames, prm)   # COLOUR EDIT
        assert ctx.tsdf_mesh_info().stale == 1 and ctx.colour_info().present == 1
        L = ctx.colour_fetch()["sums"]
        ctx.tsdf_mesh_build(1)
        ctx.colour_load(L)
        assert ctx.tsdf_mesh_info().stale == 1 and np.array_equal(ctx.colour_fetch()["sums"], L)
        ctx.tsdf_mesh_build(1)
        ctx.tsdf_integrate(sweep)   # leaves the layer alone
        assert np.array_equal(ctx.colour_fetch()["sums"], L)
        ctx.tsdf_mesh_build(1)
        ctx.colour_clear()
        assert ctx.tsdf_mesh_info().stale == 1 and not ctx.colour_fetch()["sums"].any() and ctx.colour_info().present == 1
        ctx.colour_load(L)
        ctx.tsdf_load(S, W)   # colours of another volume mean nothing
        assert not ctx.colour_fetch()["sums"].any() and ctx.colour_info().present == 1
        ctx.colour_load(L)
        ctx.tsdf_clear()
        assert not ctx.colour_fetch()["sums"].any()
        ctx.tsdf_configure(ctx.tsdf_params())   # frees it
        assert ctx.colour_info().present == 0


def test_limits_are_refused_and_write_nothing(capi, vol):
    S, W = vol
    frames = cc.frames()
    lib = capi.load_library()
    with _open(capi, S, W) as ctx:
        ctx.colour_integrate(frames, _params(capi))
        L = ctx.colour_fetch()["sums"]
        arr = (capi.LvCameraView * 3)()
        keep = []
        for i, f in enumerate(frames):
            arr[i], img = capi.camera_view(f)
            keep.append(img)
        stats = np.full(4, 7, np.uint64)
        sp = stats.ctypes.data_as(C.POINTER(C.c_uint64))

        def integrate(views=arr, n=3, **kw):
            return lib.lv_colour_integrate(ctx.h, views, n, C.byref(_params(capi, **kw)), sp)

        assert integrate(blend=1) == LV_EINVAL
        for kw in (dict(band=0), dict(band=cc.T + 1), dict(max_weight=0), dict(max_weight=65536), dict(min_weight=0), dict(zbuf_scale=17)):
            assert integrate(**kw) == LV_EINVAL, kw
        assert integrate(n=0) == LV_EINVAL and integrate(n=33) == LV_EINVAL and integrate(views=None) == LV_EINVAL
        bad = (capi.LvCameraView * 3)(*arr)
        bad[1].fx = float("nan")
        assert integrate(views=bad) == LV_EINVAL
        bad[1].fx, bad[1].image = 400.0, None
        assert integrate(views=bad) == LV_EINVAL
        assert integrate(band=cc.T) == 0 and integrate() == 0
        L = ctx.colour_fetch()["sums"]
        stats[:] = 7
        assert integrate(band=cc.T + 1) == LV_EINVAL and np.all(stats == 7)
        u32, u8 = C.POINTER(C.c_uint32), C.POINTER(C.c_uint8)
        flat = L.reshape(-1).copy()
        assert lib.lv_colour_load(ctx.h, flat.ctypes.data_as(u32), S.size - 1) == LV_EINVAL
        assert lib.lv_colour_load(ctx.h, None, S.size) == LV_EINVAL
        k = int(np.flatnonzero(L[..., 3].reshape(-1) > 0)[0])
        flat[4 * k + 1] = 255 * flat[4 * k + 3] + 1   # C > 255 * Wc
        assert lib.lv_colour_load(ctx.h, flat.ctypes.data_as(u32), S.size) == LV_EINVAL
        flat[4 * k + 1] = 0
        flat[4 * k + 3] = 65536
        assert lib.lv_colour_load(ctx.h, flat.ctypes.data_as(u32), S.size) == LV_EINVAL
        out = np.zeros(4 * S.size, np.uint32)
        assert lib.lv_colour_fetch(ctx.h, out.ctypes.data_as(u32), None, S.size - 1) == LV_EINVAL and not out.any()
        assert lib.lv_colour_fetch(ctx.h, None, None, S.size) == LV_EINVAL
        assert np.array_equal(ctx.colour_fetch()["sums"], L)   # nothing above changed the layer
        counts = ctx.tsdf_mesh_build(1)
        rgba = np.zeros((int(counts[0]), 4), np.uint8)
        assert lib.lv_mesh_colours(ctx.h, rgba.ctypes.data_as(u8), len(rgba) - 1) == LV_EINVAL and not rgba.any()
        assert lib.lv_mesh_colours(ctx.h, None, len(rgba)) == LV_EINVAL
        pts = np.zeros((2, 3), np.float32)
        assert lib.lv_colour_query(ctx.h, pts.ctypes.data_as(C.c_void_p), 8, 2, rgba.ctypes.data_as(u8)) == LV_EINVAL


def test_end_to_end_sphere(capi):
    import tsdf_cases as tc
    from limo_velo_amd import mesh

    case = tc.sphere_case(**tc.SPHERE_SMALL)
    prm_t = case["prm"]
    res = prm_t["resolution"]
    centre = np.asarray(prm_t["origin"]) + res * case["centre"]
    r = res * case["radius"]
    eye = centre + np.array([-4.0 * r, 0.0, 0.0])
    colour = (31, 200, 117)
    img = np.empty((480, 640, 3), np.uint8)
    img[:] = colour
    frame = dict(R=cc.look_at(eye, centre), t=eye.astype(np.float32), fx=400.0, fy=400.0, cx=319.63, cy=240.21, image=img)
    with capi.Context() as ctx:
        ctx.tsdf_configure(capi.default_tsdf_params(**{k: (list(v) if k == "origin" else v) for k, v in prm_t.items()}))
        for views in case["calls"]:
            mesh.integrate(ctx, views)
        prm = mesh.colour_params_for(ctx, frame, nearest=3.0 * r)
        stats = mesh.paint(ctx, [frame], prm)
        xyz, tri, counts, rgba = mesh.build(ctx, colours=True)
        vol = ctx.tsdf_fetch()
        layer = ctx.colour_fetch()["sums"]
    ref = cr.integrate(vol["S"], vol["W"], None, prm_t["origin"], res, [frame], prm)
    _check(layer, stats, ref, np.zeros_like(layer), "sphere", min_coloured=100)
    assert np.array_equal(rgba, cr.mesh_colours(vol["S"], vol["W"], layer, 1))
    near = np.linalg.norm(xyz - (centre + [-r, 0, 0]), axis=1) < 0.3 * r
    far = np.linalg.norm(xyz - (centre + [r, 0, 0]), axis=1) < 0.3 * r
    print(f"sphere: {len(xyz)} vertices, {int(near.sum())} at the near pole, {int(far.sum())} at the far pole")
    assert near.sum() > 10 and far.sum() > 5
    assert np.all(rgba[near] == colour + (255,))
    assert np.all(rgba[far, 3] == 0)
