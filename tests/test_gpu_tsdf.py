"""GPU tests of the TSDF and its mesh (lv_tsdf.hip; include/limovelo_hip.h "TSDF and mesh") against the numpy statement of the rule
in tests/tsdf_ref.py, on the shared cases of tests/tsdf_cases.py.  The rule is integer arithmetic after one quantisation step, so
everything is held to equality: S, W and stats as integers, metres as bits (NaN by isnan), vertices and indices one by one."""
import ctypes as C

import numpy as np
import pytest

import tsdf_cases as tc
import tsdf_ref as tr

pytestmark = pytest.mark.gpu

LV_OK, LV_EINVAL, LV_ESTATE = 0, -1, -4
F = np.float32


@pytest.fixture(scope="module")
def capi(lv):
    from limo_velo_amd import capi as c

    return c


@pytest.fixture(scope="module")
def ctx(capi):
    """One context for the module: every test configures the volume it needs."""
    with capi.Context() as c:
        yield c


def _configure(capi, ctx, prm):
    ctx.tsdf_configure(capi.default_tsdf_params(**prm))


def _same_mesh(got, ref):
    assert np.array_equal(got["sub"], ref["sub"])
    assert np.array_equal(got["xyz"].view(np.uint32), ref["xyz"].view(np.uint32))
    assert np.array_equal(got["tri"], ref["tri"])


def _probe_points(prm, rng, n=500):
    """World points inside the grid, outside it, on its faces, and non-finite ones."""
    lo = np.asarray(prm["origin"], np.float64)
    hi = lo + prm["resolution"] * np.array([prm["nx"], prm["ny"], prm["nz"]])
    pts = rng.uniform(lo - 1.0, hi + 1.0, (n, 3)).astype(F)
    pts[0] = lo
    pts[1] = hi
    pts[2] = (np.nan, 0, 0)
    pts[3] = (0, np.inf, 0)
    pts[4] = (1e30, 0, 0)
    return pts


@pytest.mark.parametrize("case", tc.cases(), ids=lambda c: c["name"])
def test_shared_cases(capi, ctx, case):
    prm = case["prm"]
    ref = tc.reference(case)
    _configure(capi, ctx, prm)
    assert tr.params_of(ctx.tsdf_params()) == tr.params_of(capi.default_tsdf_params(**prm))
    stats = [ctx.tsdf_integrate(views) for views in case["calls"]]
    assert [list(s) for s in stats] == [list(s) for s in ref["stats"]]
    vol = ctx.tsdf_fetch(S=True, W=True, metres=True)
    assert np.array_equal(vol["S"], ref["S"]) and np.array_equal(vol["W"], ref["W"])
    assert tr.same_metres(vol["metres"], tr.metres(prm, ref["S"], ref["W"]))
    pts = _probe_points(prm, np.random.default_rng(3))
    m, w = ctx.tsdf_query(pts)
    rm, rw = tr.query(prm, ref["S"], ref["W"], pts)
    assert tr.same_metres(m, rm) and np.array_equal(w, rw) and np.isnan(m[:5][[1, 2, 3, 4]]).all()
    counts = ctx.tsdf_mesh_build(case["min_weight"])
    assert list(counts) == list(ref["mesh"]["counts"])
    _same_mesh(ctx.tsdf_mesh_fetch(), ref["mesh"])


def test_the_scratch_is_left_zero_and_calls_accumulate(capi, ctx):
    """The same sweep twice equals the reference's two calls: the fold left nothing behind in the scratch."""
    prm = tc.grid_params(33, 17, 9, carve=1)
    view = tc.random_view(np.random.default_rng(9), tc.INSIDE)
    S, W = tr.empty(prm)
    _configure(capi, ctx, prm)
    for _ in range(2):
        S, W, st = tr.integrate(prm, S, W, [view])
        assert list(ctx.tsdf_integrate([view])) == list(st)
    vol = ctx.tsdf_fetch()
    assert np.array_equal(vol["S"], S) and np.array_equal(vol["W"], W)


def test_fetch_load_fetch_is_the_identity_and_load_refuses(capi, ctx):
    case = tc.cases()[1]
    prm, ref = case["prm"], tc.reference(case)
    _configure(capi, ctx, prm)
    for views in case["calls"]:
        ctx.tsdf_integrate(views)
    a = ctx.tsdf_fetch()
    assert np.array_equal(a["S"], ref["S"])
    ctx.tsdf_clear()
    assert not ctx.tsdf_fetch(S=False)["W"].any()
    ctx.tsdf_load(a["S"], a["W"])
    b = ctx.tsdf_fetch()
    assert np.array_equal(a["S"], b["S"]) and np.array_equal(a["W"], b["W"])
    T = prm["trunc_cells"] * 256
    for i, (s, w) in enumerate(((0, -1), (0, prm["max_weight"] + 1), (T * 2 + 1, 2), (-T - 1, 1), (1, 0))):
        S, W = a["S"].copy(), a["W"].copy()
        S.reshape(-1)[17 + i], W.reshape(-1)[17 + i] = s, w
        with pytest.raises(capi.LvError):
            ctx.tsdf_load(S, W)
    with pytest.raises(capi.LvError):
        ctx.tsdf_load(a["S"].reshape(-1)[:-1], a["W"].reshape(-1)[:-1])
    b = ctx.tsdf_fetch()
    assert np.array_equal(a["S"], b["S"]) and np.array_equal(a["W"], b["W"])   # (a refused load changed nothing)
    S, W = a["S"].copy(), a["W"].copy()
    S.reshape(-1)[5], W.reshape(-1)[5] = -T * prm["max_weight"], prm["max_weight"]   # (on the limits: accepted)
    ctx.tsdf_load(S, W)
    assert ctx.tsdf_fetch()["S"].reshape(-1)[5] == -T * prm["max_weight"]


def test_stale_follows_the_volume_and_an_unobserved_grid_meshes_to_nothing(capi, ctx):
    case = tc.sphere_case(**tc.SPHERE_SMALL)
    _configure(capi, ctx, case["prm"])
    assert ctx.tsdf_mesh_info().built == 0
    with pytest.raises(capi.LvError):
        ctx.tsdf_mesh_fetch()
    assert list(ctx.tsdf_mesh_build()) == [0, 0, 0, 0]      # (LV_OK on a volume nobody observed)
    i = ctx.tsdf_mesh_info()
    assert (i.built, i.stale, i.vertices, i.triangles) == (1, 0, 0, 0)
    m = ctx.tsdf_mesh_fetch()
    assert m["xyz"].shape == (0, 3) and m["tri"].shape == (0, 3)
    ctx.tsdf_integrate(case["calls"][0])
    assert ctx.tsdf_mesh_info().stale == 1
    counts = ctx.tsdf_mesh_build()
    i = ctx.tsdf_mesh_info()
    assert (i.built, i.stale, i.min_weight, i.vertices, i.triangles, i.active_cells, i.refused_edges) == (1, 0, 1, *[int(c) for c in counts])
    before = ctx.tsdf_mesh_fetch()
    vol = ctx.tsdf_fetch()
    ctx.tsdf_load(vol["S"], vol["W"])
    assert ctx.tsdf_mesh_info().stale == 1
    ctx.tsdf_mesh_build(1)
    ctx.tsdf_clear()
    i = ctx.tsdf_mesh_info()
    assert (i.built, i.stale, int(i.vertices)) == (1, 1, int(counts[0]))
    _same_mesh(ctx.tsdf_mesh_fetch(), before)               # (a snapshot: the cleared volume did not change it)
    ctx.tsdf_mesh_clear()
    assert ctx.tsdf_mesh_info().built == 0
    ctx.tsdf_mesh_build()
    _configure(capi, ctx, case["prm"])                      # (configure frees the mesh)
    assert ctx.tsdf_mesh_info().built == 0


def test_refusals_and_their_order(capi):
    lib = capi.load_library()
    case = tc.sphere_case(**tc.SPHERE_SMALL)
    prm = case["prm"]
    n = prm["nx"] * prm["ny"] * prm["nz"]
    stats = (C.c_uint64 * 4)(7, 7, 7, 7)
    f3 = (C.c_float * 3)(5.0, 5.0, 5.0)
    i3 = (C.c_int32 * 3)(4, 4, 4)
    u3 = (C.c_uint32 * 3)(6, 6, 6)
    arr, keep = capi.view_array(case["calls"][0])
    with capi.Context() as c:
        h = c.h
        info = capi.MeshInfo()
        p = capi.TsdfParams()
        # LV_ESTATE before configure, whatever the arguments are
        assert lib.lv_tsdf_integrate(h, None, 0, stats) == LV_ESTATE
        assert lib.lv_tsdf_query(h, None, 0, 1, None, None) == LV_ESTATE
        assert lib.lv_tsdf_fetch(h, None, None, None, 0) == LV_ESTATE
        assert lib.lv_tsdf_load(h, None, None, 0) == LV_ESTATE
        assert lib.lv_tsdf_clear(h) == LV_ESTATE
        assert lib.lv_tsdf_get_params(h, C.byref(p)) == LV_ESTATE
        assert lib.lv_tsdf_mesh_build(h, 0, stats) == LV_ESTATE
        assert lib.lv_tsdf_mesh_fetch(h, None, None, None, 0, 0) == LV_ESTATE
        assert lib.lv_tsdf_mesh_info(h, C.byref(info)) == LV_ESTATE
        assert lib.lv_tsdf_mesh_clear(h) == LV_ESTATE
        # a refused configure leaves the context unconfigured; the parameters come before the context
        bad = capi.default_tsdf_params(**dict(prm, trunc_cells=17))
        assert lib.lv_tsdf_configure(h, C.byref(bad)) == LV_EINVAL and lib.lv_tsdf_clear(h) == LV_ESTATE
        assert lib.lv_tsdf_configure(None, C.byref(bad)) == LV_EINVAL and "trunc_cells" in lib.lv_last_error().decode()
        c.tsdf_configure(capi.default_tsdf_params(**prm))
        # arguments outside the limits: LV_EINVAL, nothing touched
        assert lib.lv_tsdf_integrate(h, None, 1, stats) == LV_EINVAL
        assert lib.lv_tsdf_integrate(h, arr, 0, stats) == LV_EINVAL
        assert lib.lv_tsdf_integrate(h, arr, 33, stats) == LV_EINVAL
        big = (capi.View * 2)()
        for v in big:
            v.R[:] = [1, 0, 0, 0, 1, 0, 0, 0, 1]
            v.points, v.stride, v.n = keep[0].ctypes.data, 12, 2 ** 23 + 1    # (2^24 + 2 returns in all; judged before any is read)
        assert lib.lv_tsdf_integrate(h, big, 2, stats) == LV_EINVAL and "too many returns" in lib.lv_last_error().decode()
        nanR = (capi.View * 1)()
        nanR[0].R[0] = float("nan")
        assert lib.lv_tsdf_integrate(h, nanR, 1, stats) == LV_EINVAL
        assert lib.lv_tsdf_query(h, f3, 12, 1, None, None) == LV_EINVAL
        assert lib.lv_tsdf_query(h, f3, 8, 1, f3, i3) == LV_EINVAL
        assert lib.lv_tsdf_query(h, None, 12, 1, f3, i3) == LV_EINVAL
        assert lib.lv_tsdf_fetch(h, None, None, None, n) == LV_EINVAL
        assert lib.lv_tsdf_fetch(h, i3, None, None, n - 1) == LV_EINVAL
        assert lib.lv_tsdf_load(h, i3, i3, 3) == LV_EINVAL
        assert lib.lv_tsdf_load(h, None, None, n) == LV_EINVAL
        assert lib.lv_tsdf_get_params(h, None) == LV_EINVAL
        assert lib.lv_tsdf_mesh_build(h, 0, stats) == LV_EINVAL
        assert lib.lv_tsdf_mesh_info(h, None) == LV_EINVAL
        assert lib.lv_tsdf_mesh_fetch(h, f3, i3, u3, 1, 1) == LV_ESTATE     # (no mesh yet)
        assert list(stats) == [7, 7, 7, 7] and list(f3) == [5.0] * 3 and list(i3) == [4] * 3 and list(u3) == [6] * 3
        assert not c.tsdf_fetch(S=False)["W"].any() and c.tsdf_mesh_info().built == 0
        # capacities too small
        c.tsdf_integrate(case["calls"][0])
        V, Fc = (int(v) for v in c.tsdf_mesh_build()[:2])
        assert V > 3 and Fc > 3
        assert lib.lv_tsdf_mesh_fetch(h, None, None, None, V, Fc) == LV_EINVAL
        assert lib.lv_tsdf_mesh_fetch(h, f3, None, None, V - 1, Fc) == LV_EINVAL
        assert lib.lv_tsdf_mesh_fetch(h, None, i3, None, V - 1, Fc) == LV_EINVAL
        assert lib.lv_tsdf_mesh_fetch(h, None, None, u3, V, Fc - 1) == LV_EINVAL
        assert list(f3) == [5.0] * 3 and list(i3) == [4] * 3 and list(u3) == [6] * 3
        tri = np.zeros((Fc, 3), np.uint32)
        assert lib.lv_tsdf_mesh_fetch(h, None, None, tri.ctypes.data_as(C.POINTER(C.c_uint32)), 0, Fc) == LV_OK   # (no vertex array: its capacity is not judged)
        assert np.array_equal(tri, tc.reference(case)["mesh"]["tri"])
        # only one of metres / weight
        pts = np.array([[0.0, 3.0, 2.0]], F)
        m = np.zeros(1, F)
        assert lib.lv_tsdf_query(h, pts.ctypes.data_as(C.c_void_p), 12, 1, m.ctypes.data_as(C.POINTER(C.c_float)), None) == LV_OK
        assert lib.lv_tsdf_query(h, None, 0, 0, f3, None) == LV_OK      # (no points: nothing to do)


def _read_ply(path):
    """A small PLY reader: (vertices [V, 3] f32, triangles [F, 3] int32) of an ASCII or binary little-endian file."""
    raw = open(path, "rb").read()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    head = raw[:end].decode("ascii").split("\n")
    assert head[0] == "ply"
    fmt = head[1].split()[1]
    nv = int([l for l in head if l.startswith("element vertex")][0].split()[2])
    nf = int([l for l in head if l.startswith("element face")][0].split()[2])
    assert [l for l in head if l.startswith("property")] == ["property float x", "property float y", "property float z",
                                                            "property list uchar int vertex_indices"]
    body = raw[end:]
    if fmt == "ascii":
        rows = [l.split() for l in body.decode("ascii").split("\n") if l]
        v = np.array(rows[:nv], np.float64).astype(F).reshape(-1, 3)
        f = np.array(rows[nv:nv + nf], np.int64).reshape(-1, 4)
        assert len(rows) == nv + nf
    else:
        assert fmt == "binary_little_endian"
        v = np.frombuffer(body, "<f4", 3 * nv).reshape(-1, 3)
        f = np.frombuffer(body, np.dtype([("n", "u1"), ("i", "<i4", 3)]), nf, 12 * nv)
        assert len(body) == 12 * nv + 13 * nf
        f = np.concatenate([f["n"][:, None].astype(np.int64), f["i"].astype(np.int64)], axis=1).reshape(-1, 4)
    assert np.all(f[:, 0] == 3)
    return v, f[:, 1:].astype(np.int32)


def test_mesh_helpers_and_ply_round_trip(capi, ctx, tmp_path):
    from limo_velo_amd import mesh

    case = tc.sphere_case(**tc.SPHERE_SMALL)
    ref = tc.reference(case)
    _configure(capi, ctx, case["prm"])
    stats = mesh.integrate(ctx, case["calls"][0])
    assert list(stats) == list(ref["stats"][0])
    v, t, counts = mesh.build(ctx)
    assert list(counts) == [680, 1356, 680, 0]
    assert np.array_equal(v.view(np.uint32), ref["mesh"]["xyz"].view(np.uint32)) and np.array_equal(t, ref["mesh"]["tri"])
    for binary in (True, False):
        path = str(tmp_path / ("mesh_%d.ply" % binary))
        mesh.save_ply(path, v, t, binary=binary)
        rv, rt = _read_ply(path)
        assert np.array_equal(rv.view(np.uint32), v.view(np.uint32)) and np.array_equal(rt, t.astype(np.int32))
    with pytest.raises(ValueError):
        mesh.save_ply(str(tmp_path / "bad.ply"), v[:10], t)
    # distance(): the sensor's own voxel is in front of the surface, a point beyond the sphere was never observed
    prm = case["prm"]
    centre = np.asarray(prm["origin"]) + prm["resolution"] * case["centre"]
    m, w = mesh.distance(ctx, np.array([centre + [prm["resolution"] * 5.0, 0, 0], centre + [prm["resolution"] * 9.6, 0, 0]], F))
    rm, rw = tr.query(prm, ref["S"], ref["W"], np.array([centre + [prm["resolution"] * 5.0, 0, 0], centre + [prm["resolution"] * 9.6, 0, 0]], F))
    assert tr.same_metres(m, rm) and np.array_equal(w, rw) and m[0] > 0 and w[0] > 0 and w[1] == 0
    # save / load of the volume
    path = str(tmp_path / "volume")   # (no extension: save and load add the same one)
    mesh.save(ctx, path)
    _configure(capi, ctx, tc.grid_params(5, 4, 3))
    p = mesh.load(ctx, path)
    assert tr.params_of(p) == tr.params_of(capi.default_tsdf_params(**prm))
    vol = ctx.tsdf_fetch()
    assert np.array_equal(vol["S"], ref["S"]) and np.array_equal(vol["W"], ref["W"])
    v2, t2, _ = mesh.build(ctx)
    assert np.array_equal(v2.view(np.uint32), v.view(np.uint32)) and np.array_equal(t2, t)
