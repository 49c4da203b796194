"""GPU tests of the depth fusion (lv_depth.hip; include/limovelo_hip.h "Depth fusion") against the numpy statement of the rule in
tests/depth_ref.py, by EQUALITY on S, W and all four stats: the rule is a fixed sequence of single f32 operations and integers
after them, so there is no tolerance and no undecided share.  The scene is tests/depth_cases.py's (tests/test_depth_ref.py holds
that it reaches every class of the rule)."""
import ctypes as C

import numpy as np
import pytest

import depth_cases as dc
import depth_ref as dr

pytestmark = pytest.mark.gpu

LV_EINVAL, LV_ESTATE = -1, -4
F = np.float32
MAX_WEIGHT = 10000


@pytest.fixture(scope="module")
def capi(lv):
    from limo_velo_amd import capi as c

    return c


def _open(capi, shape=(dc.NZ, dc.NY, dc.NX), origin=dc.ORIGIN, resolution=dc.RES, max_weight=MAX_WEIGHT, **kw):
    ctx = capi.Context()
    nz, ny, nx = shape
    ctx.tsdf_configure(capi.default_tsdf_params(origin=[float(v) for v in origin], resolution=resolution, nx=nx, ny=ny, nz=nz,
                                                trunc_cells=dc.TRUNC_CELLS, max_weight=max_weight, **kw))
    return ctx


def _cp(capi, p):
    return capi.default_depth_params(min_depth=p.min_depth, max_depth=p.max_depth, max_norm_radius=p.max_norm_radius, carve=p.carve)


def _call(capi, ctx, frames, prm, S, W, what, origin=dc.ORIGIN, resolution=dc.RES, max_weight=MAX_WEIGHT, touched=1):
    """One lv_depth_integrate on ctx, whose volume is (S, W), held to the reference of that call; returns the volume after."""
    stats = ctx.tsdf_integrate_depth(frames, _cp(capi, prm))
    got = ctx.tsdf_fetch()
    ref = dr.integrate(S, W, origin, resolution, dc.TRUNC_CELLS, max_weight, frames, prm)
    dS, dW = int((got["S"] != ref["S"]).sum()), int((got["W"] != ref["W"]).sum())
    print(f"{what}: stats {stats} (reference {ref['stats']}), {dS} voxels differ in S, {dW} in W, {int((got['W'] > 0).sum())} observed")
    assert np.array_equal(stats, ref["stats"]), (what, stats, ref["stats"])
    assert np.array_equal(got["W"], ref["W"]) and np.array_equal(got["S"], ref["S"]), what
    assert int(stats[3]) >= touched, what
    return got["S"], got["W"]


def _zeros(shape=(dc.NZ, dc.NY, dc.NX)):
    return np.zeros(shape, np.int32), np.zeros(shape, np.int32)


@pytest.mark.parametrize("carve", [0, 1])
def test_the_scene(capi, carve):
    with _open(capi) as ctx:
        S, W = _call(capi, ctx, [dc.frame()], dc.params(carve=carve), *_zeros(), f"scene, carve {carve}", touched=4000)
    T = dc.TRUNC_CELLS * 256
    assert W.max() == 1 and S.min() < -T // 2 and ((S == T).sum() > 5000) == bool(carve)   # (the free space in front of the band)


def test_three_views_in_one_call_and_in_three(capi):
    fr, prm = dc.frames3(), dc.params(carve=1)
    with _open(capi) as one, _open(capi) as three:
        S1, W1 = _call(capi, one, fr, prm, *_zeros(), "three views, one call")
        S, W = _zeros()
        for n, f in enumerate(fr[::-1]):
            S, W = _call(capi, three, [f], prm, S, W, f"three views, call {n}")
    assert np.array_equal(S, S1) and np.array_equal(W, W1) and W1.max() == 3   # below max_weight neither order nor split matters


def test_the_folds_scaling_branch(capi):
    fr, prm = dc.frames3() + [dc.frame()], dc.params()
    with _open(capi, max_weight=3) as ctx:
        S, W = _call(capi, ctx, fr[:2], prm, *_zeros(), "max_weight 3, call 0", max_weight=3)
        assert W.max() == 2
        S, W = _call(capi, ctx, fr[2:], prm, S, W, "max_weight 3, call 1", max_weight=3)
        assert W.max() == 3 and (dr.integrate(*_zeros(), dc.ORIGIN, dc.RES, dc.TRUNC_CELLS, 10, fr, prm)["W"] == 4).sum() > 500   # voxels that were scaled
        S, W = _call(capi, ctx, fr[:2], prm, S, W, "max_weight 3, call 2", max_weight=3)   # ... and scaled from the cap itself
        assert W.max() == 3


@pytest.mark.parametrize("variant", ["f32", "padded", "distorted"])
def test_formats_and_layouts(capi, variant):
    f = {"f32": dc.frame_f32, "padded": dc.frame_padded, "distorted": dc.frame_distorted}[variant]()
    with _open(capi) as ctx:
        S, W = _call(capi, ctx, [f], dc.params(), *_zeros(), variant, touched=3000)
    if variant == "padded":   # the padding is never read: the packed image's volume
        ref = dr.integrate(*_zeros(), dc.ORIGIN, dc.RES, dc.TRUNC_CELLS, MAX_WEIGHT, [dc.frame()], dc.params())
        assert np.array_equal(S, ref["S"]) and np.array_equal(W, ref["W"])


@pytest.mark.parametrize("shape,origin", [((2, 3, 5), (-0.9, 0.0, -0.1)), ((25, 41, 49), dc.ORIGIN)])
def test_volume_shapes(capi, shape, origin):
    """5 x 3 x 2: smaller than any tile.  49 x 41 x 25: no dimension a multiple of anything, tails in x, y and z."""
    with _open(capi, shape, origin) as ctx:
        S, W = _call(capi, ctx, dc.frames3(), dc.params(carve=1), *_zeros(shape), f"{shape}", origin=origin, touched=20)
    assert (W > 0).sum() > 20


def test_one_pixel_image(capi):
    with _open(capi) as ctx:
        S, W = _call(capi, ctx, [dc.frame_pixel()], dc.params(), *_zeros(), "1 x 1 image", touched=3)
    k, j, i = np.nonzero(W)
    assert set(k) == {12} and set(j) == {20}   # the voxels on the optical axis


def test_corner_and_nothing(capi):
    corner, prm = dc.frame_corner(), dc.params(max_depth=1.2)
    with _open(capi) as ctx:
        S, W = _call(capi, ctx, [corner], prm, *_zeros(), "corner", touched=50)
        S, W = _call(capi, ctx, [corner, dc.frame_nothing(), dc.frame()], dc.params(), S, W, "corner, nothing and the scene", touched=4000)
        ctx.tsdf_mesh_build(1)
        assert ctx.tsdf_mesh_info().stale == 0
        stats = ctx.tsdf_integrate_depth([dc.frame_nothing()], _cp(capi, dc.params()))   # nobody sees a voxel
        got = ctx.tsdf_fetch()
        assert not stats.any() and np.array_equal(got["S"], S) and np.array_equal(got["W"], W)
        assert ctx.tsdf_mesh_info().stale == 1   # the edit is marked before the store is asked


def test_32_views(capi):
    with _open(capi) as ctx:
        S, W = _call(capi, ctx, dc.frames32(), dc.params(carve=1), *_zeros(), "32 views", touched=6000)
    assert W.max() > 16
    with _open(capi) as ctx:   # one more is refused, nothing written
        with pytest.raises(capi.LvError, match="error -1: lv_depth_integrate: n_views = 33"):
            ctx.tsdf_integrate_depth(dc.frames32() + [dc.frame()], _cp(capi, dc.params()))
        assert not ctx.tsdf_fetch()["W"].any()


def test_on_top_of_a_sweep(capi):
    import tsdf_cases as tc

    case = next(c for c in tc.cases() if c["name"] == "33x17x9-carve0-3views")
    p = case["prm"]
    ref = tc.reference(case)
    frame = dc.frame_flat((0.0, 1.5, 1.0), 2500, yaw=0.2, pitch=0.1)
    shape = (p["nz"], p["ny"], p["nx"])
    with capi.Context() as ctx:
        ctx.tsdf_configure(capi.default_tsdf_params(**{k: (list(v) if k == "origin" else v) for k, v in p.items()}))
        for views in case["calls"]:
            ctx.tsdf_integrate(views)
        got = ctx.tsdf_fetch()
        assert np.array_equal(got["S"], ref["S"]) and np.array_equal(got["W"], ref["W"]) and (ref["W"] > 0).sum() > 500
        S, W = _call(capi, ctx, [frame], dc.params(carve=1), ref["S"], ref["W"], "on a sweep", origin=p["origin"], resolution=p["resolution"],
                     max_weight=p["max_weight"], touched=300)
    both = (np.asarray(ref["W"]) > 0) & (W > np.asarray(ref["W"]))
    print(f"on a sweep: {int(both.sum())} voxels hold evidence of both")
    assert both.sum() > 50 and shape == W.shape


def test_after_a_recentre(capi):
    from colour_ref import shift_layer

    d = (3, -2, 1)
    prm = dc.params(carve=1)
    with _open(capi) as ctx:
        S, W = _call(capi, ctx, [dc.frame()], prm, *_zeros(), "before the shift")
        ctx.volume_recentre(capi.LV_VOLUME_SURFACE, d)
        origin = [float(x) for x in ctx.tsdf_params().origin]
        assert origin != list(dc.ORIGIN)
        S, W = shift_layer(S, d), shift_layer(W, d)
        got = ctx.tsdf_fetch()
        assert np.array_equal(got["S"], S) and np.array_equal(got["W"], W)
        S2, W2 = _call(capi, ctx, [dc.frame(dc.POSES[1])], prm, S, W, "after the shift", origin=origin, touched=4000)
    stay = dr.integrate(S, W, dc.ORIGIN, dc.RES, dc.TRUNC_CELLS, MAX_WEIGHT, [dc.frame(dc.POSES[1])], prm)
    assert not np.array_equal(stay["W"], W2)   # (the origin of before gives another volume: the centres did move)


def test_states_and_stale_rows(capi):
    frames, prm = [dc.frame()], _cp(capi, dc.params())
    with capi.Context() as ctx:   # before lv_tsdf_configure
        with pytest.raises(capi.LvError, match="error -4: no TSDF volume"):
            ctx.tsdf_integrate_depth(frames, prm)
        with pytest.raises(capi.LvError, match="error -1: lv_depth_integrate: carve = 2"):   # the arguments come first
            ctx.tsdf_integrate_depth(frames, capi.default_depth_params(carve=2))
    rng = np.random.default_rng(8)
    _, _, t = dc.POSE
    frm, to = np.array([t], F), np.array([[2.0, t[1], t[2]]], F)
    with _open(capi) as ctx:
        Wc = rng.integers(0, 5, (dc.NZ, dc.NY, dc.NX, 1))
        L = np.concatenate([rng.integers(0, 256, (dc.NZ, dc.NY, dc.NX, 3)) * Wc, Wc], axis=-1).astype(np.uint32)
        ctx.colour_load(L)
        ctx.tsdf_mesh_build(1)
        before = ctx.tsdf_raycast(frm, to)[0]
        assert before["status"][0] == capi.LV_SURF_CLEAR and ctx.tsdf_mesh_info().stale == 0
        # a refused call changes nothing and marks nothing
        view, keep = capi.depth_view(frames[0])
        stats = np.full(4, 7, np.uint64)
        rc = ctx.lib.lv_depth_integrate(ctx.h, (capi.DepthView * 1)(view), 1, C.byref(capi.default_depth_params(max_depth=0.1)),
                                        stats.ctypes.data_as(C.POINTER(C.c_uint64)))
        assert rc == LV_EINVAL and np.all(stats == 7) and ctx.tsdf_mesh_info().stale == 0 and not ctx.tsdf_fetch()["W"].any()
        st = ctx.tsdf_integrate_depth(frames, prm)
        assert st[3] > 4000
        assert ctx.tsdf_mesh_info().stale == 1                        # SURFACE EDIT
        assert np.array_equal(ctx.colour_fetch()["sums"], L)          # the colour layer is left alone, bit for bit
        after = ctx.tsdf_raycast(frm, to)[0]                          # the packed states were built anew
        print(f"ray along the optical axis: status {before['status'][0]} before, {after['status'][0]} after, depth {after['depth'][0]} sub-units")
        assert after["status"][0] == capi.LV_SURF_HIT
        assert ctx.lib.lv_depth_integrate(ctx.h, (capi.DepthView * 1)(view), 1, C.byref(prm), None) == 0   # stats may be NULL


def test_round_trip_through_a_rendered_view(capi):
    from limo_velo_amd import mesh

    yaw, pitch, t = dc.POSE
    R = dc.rot(yaw, pitch).astype(F)
    with _open(capi) as a, _open(capi) as b:
        mesh.integrate_depth(a, dc.frames3(), _cp(capi, dc.params()))
        f = mesh.render_frame(a, R, t, dc.FOCAL, dc.FOCAL, dc.CX, dc.CY, dc.WIDTH, dc.HEIGHT, max_range=6.0)
        d = f["depth"]
        hit = np.isfinite(d)
        print(f"rendered frame: {int(hit.sum())} of {d.size} pixels hit, depth {np.nanmin(d):.3f}..{np.nanmax(d):.3f} m")
        assert d.dtype == F and d.shape == (dc.HEIGHT, dc.WIDTH) and hit.sum() > d.size // 2 and np.isnan(d).any()
        S, W = _call(capi, b, [f], dc.params(), *_zeros(), "round trip", touched=2000)
        va = a.tsdf_fetch()   # (what was rendered from a's surface is a's surface again: the figure below is printed, not held)
    both = (W > 0) & (va["W"] > 0)
    da, db = va["S"][both] / va["W"][both], S[both] / W[both]
    near = (np.abs(da) < 128) & (np.abs(db) < 128)
    print(f"round trip: {int(both.sum())} voxels in both, {int(near.sum())} near the surface, max |difference| {np.abs(da - db)[near].max():.1f} sub-units")
    assert near.sum() > 300


def test_a_wall_is_where_it_was_measured(capi):
    """An axis-aligned camera at x = tx looks along +x at a fronto-parallel wall: every pixel measures 2000 mm, D = 2.0f exactly.
    Every mesh vertex lies within 3 sub-units (3 / 256 of a voxel) of x = tx + 2 in x.  Derivation, in sub-units, d* the true
    distance of a voxel centre in front of the wall:
      - R is a signed permutation, so z = (1 * dx + 0 * dy) + 0 * dz = dx exactly, and s = floorf(((D - z) / res) * 256) lies in
        (d* - 1, d*] up to the f32 roundings of the centre, the subtraction and the division (about 1e-3 sub-units together);
      - along x the centres are 256 sub-units apart, so the voxels A (s_A >= 0) and B (s_B < 0) on both sides of the wall have the
        same fraction of d*: s_A - s_B = 256 and the crossing t = (256 s_A) / 256 = s_A, unless the roundings above put one of the
        two floors on the other side of an integer; then s_A - s_B is 255 or 257, and t = floor(256 s_A / (s_A - s_B)) is less
        than one sub-unit from s_A, and the truncating division takes less than one more: t - d* in (-2, 0] with either;
      - the vertex is the truncated mean of its cell's crossings (here the four edges along x): less than one sub-unit more,
        (-3, 0]; its metres are one more f32 rounding, far below a sub-unit."""
    tx = float(F(-1.93))
    f = dc.frame_flat((tx, 0.03, 0.02), 2000)
    assert F(2000) * F(0.001) == F(2.0) and np.array_equal(f["R"], dc.AXES.astype(F))
    with _open(capi) as ctx:
        _call(capi, ctx, [f], dc.params(), *_zeros(), "wall", touched=2000)
        counts = ctx.tsdf_mesh_build(1)
        m = ctx.tsdf_mesh_fetch()
    wall = tx + 2.0
    wall_sub = (wall - float(F(dc.ORIGIN[0]))) / float(F(dc.RES)) * 256.0
    err = m["sub"][:, 0].astype(np.float64) - wall_sub
    err_m = m["xyz"][:, 0].astype(np.float64) - wall
    print(f"wall: {int(counts[0])} vertices, {int(counts[1])} triangles, x - wall in [{err.min():.3f}, {err.max():.3f}] sub-units, "
          f"[{err_m.min():.2e}, {err_m.max():.2e}] m")
    assert counts[0] > 500 and counts[1] > 500
    assert np.abs(err).max() <= 3.0
    assert np.abs(err_m).max() <= 3.0 / 256.0 * dc.RES
