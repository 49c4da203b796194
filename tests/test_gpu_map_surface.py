"""GPU tests of lv_map_normals / lv_map_remove_outliers (lv_surface.hip) against the numpy statement of both rules in
tests/surface_ref.py: neighbour sets exact ((d2 f32, id) order), everything after within the rounding of f64 work and one f32
rounding of the outputs."""
import ctypes as C
import time

import numpy as np
import pytest
from scipy.spatial import cKDTree

import surface_ref as sr

pytestmark = pytest.mark.gpu

LV_EINVAL = -1
ANGLE_TOL = 5e-7      # rad: the f32 rounding of the output (~1e-7) plus the conditioning term (<= 1e-12 / 1e-3)
GAP_MIN = 1e-3        # normals are compared where the reference's (l1 - l0) / l2 is at least this
SIGN_BAND = 1e-6      # the sign may differ where the deciding quantity is this close (relative) to its tie


@pytest.fixture(scope="module")
def capi(lv):
    from limo_velo_amd import capi as c

    return c


@pytest.fixture(scope="module")
def scene():
    from limo_velo_amd import synth

    return synth.make_scene(100_000, 4_000)


@pytest.fixture(scope="module")
def ghosts(scene):
    """500 points each >= 1 m from every other point of the map and from each other."""
    xyz = scene["map_xyz"].astype(np.float64)
    tree = cKDTree(xyz)
    rng = np.random.default_rng(77)
    lo, hi = xyz.min(axis=0), xyz.max(axis=0)
    out = np.empty((0, 3))
    while len(out) < 500:
        c = rng.uniform(lo, hi, (4000, 3)).astype(np.float32).astype(np.float64)
        c = c[tree.query(c)[0] >= 1.05]
        for p in c:
            if len(out) == 0 or np.min(np.linalg.norm(out - p, axis=1)) >= 1.05:
                out = np.vstack([out, p])
            if len(out) == 500:
                break
    g = out.astype(np.float32)
    both = np.concatenate([scene["map_xyz"], g])
    d, _ = cKDTree(both.astype(np.float64)).query(g.astype(np.float64), k=2)
    assert np.all(d[:, 1] >= 1.0)
    return g


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _angle(a, b):
    return np.arcsin(np.minimum(np.linalg.norm(np.cross(a, b), axis=1), 1.0))


def _check_normals(out, ref, sel=None, label="", cv_floor=0.0):
    """Holds a device result to the reference on the points `sel` (default: all); returns the share of points left out.
    cv_floor: an absolute error of the curvature taken off before the 2 ulp (the duplicates case only, see there)."""
    m = len(ref["n_used"])
    sel = np.ones(m, bool) if sel is None else sel
    assert np.array_equal(out["n_used"][sel], ref["n_used"][sel])
    few = ref["few"]
    # mean distance: 2 f32 ulp
    md_ref = ref["mean_dist"].astype(np.float32)
    fin = np.isfinite(md_ref) & sel
    err_md = np.abs(out["mean_dist"][fin].astype(np.float64) - ref["mean_dist"][fin]) / sr.ulp32(md_ref[fin])
    assert np.array_equal(np.isinf(out["mean_dist"][sel]), np.isinf(md_ref[sel]))
    # curvature: NaN where too few neighbours, else 2 f32 ulp
    assert np.all(np.isnan(out["curvature"][few & sel])) and not np.any(np.isnan(out["curvature"][~few & sel]))
    assert np.all(out["normals"][few & sel] == 0)
    ok = ~few & sel
    cv_ref = ref["curvature"].astype(np.float32)
    err_cv = np.maximum(np.abs(out["curvature"][ok].astype(np.float64) - ref["curvature"][ok]) - cv_floor, 0.0) / \
        sr.ulp32(np.maximum(cv_ref[ok], np.float32(1e-30)))
    # normals: where the reference's gap allows
    cmp_ = ok & (ref["gap"] >= GAP_MIN)
    nd = out["normals"].astype(np.float64)
    ang = _angle(nd[cmp_], ref["normals"][cmp_])
    same = np.einsum("ij,ij->i", nd[cmp_], ref["normals"][cmp_]) > 0
    band = ref["sign_margin"][cmp_] <= SIGN_BAND
    left_out = (ok & ~cmp_).sum() + band.sum()
    print(f"{label} points {int(sel.sum())}: mean_dist err max {err_md.max() if len(err_md) else 0:.3f} ulp, curvature err max "
          f"{err_cv.max() if len(err_cv) else 0:.3f} ulp, normal angle max {ang.max() if len(ang) else 0:.3e} rad, smallest gap "
          f"{ref['gap'][ok].min() if ok.any() else float('nan'):.3e}, left out {int(left_out)}")
    assert np.all(err_md <= 2.0), err_md.max()
    assert np.all(err_cv <= 2.0), err_cv.max()
    assert np.all(ang <= ANGLE_TOL), ang.max()
    assert np.all(same | band), int((~(same | band)).sum())
    assert np.all(np.abs(np.linalg.norm(nd[ok], axis=1) - 1.0) <= 2e-7)
    return left_out / max(int(sel.sum()), 1)


@pytest.mark.parametrize("k", [5, 10, 32])
@pytest.mark.parametrize("orient", [0, 1])
def test_normals_match_the_reference(capi, scene, k, orient):
    xyz = scene["map_xyz"]
    vp = (3.0, -2.0, 1.5)
    with capi.Context() as ctx:
        ctx.map_build(xyz)
        out = ctx.map_normals(capi.default_surface_params(k=k, orient=orient, viewpoint=vp, min_neighbours=min(5, k)))
    ref = sr.normals(xyz, k=k, max_dist=2.0, min_neighbours=min(5, k), orient=orient, viewpoint=vp)
    share = _check_normals(out, ref, label=f"k={k} orient={orient}")
    assert share <= 0.01, share


def test_optional_outputs_and_capacity(capi, scene):
    xyz = scene["map_xyz"][:20_000]
    lib = capi.load_library()
    with capi.Context() as ctx:
        ctx.map_build(xyz)
        full = ctx.map_normals()
        md = np.zeros(len(xyz), np.float32)
        p = capi.default_surface_params()
        ctx._check(lib.lv_map_normals(ctx.h, C.byref(p), None, None, md.ctypes.data_as(C.POINTER(C.c_float)), None, len(xyz)))
        assert np.array_equal(_bits(md), _bits(full["mean_dist"]))
        again = ctx.map_normals()
        for key in full:   # bitwise reproducible
            assert np.array_equal(full[key].view(np.uint8), again[key].view(np.uint8)), key
        assert lib.lv_map_normals(ctx.h, C.byref(p), None, None, md.ctypes.data_as(C.POINTER(C.c_float)), None, len(xyz) - 1) == LV_EINVAL
    with capi.Context() as ctx:   # an unbuilt map: nothing to do
        assert ctx.map_normals()["n_used"].shape == (0,)
        assert ctx.map_remove_outliers()[0] == 0


def test_lattice_ties_go_by_index(capi):
    g = np.arange(12, dtype=np.float32) * np.float32(0.25)
    xyz = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    xyz = xyz[np.random.default_rng(3).permutation(len(xyz))]
    with capi.Context() as ctx:
        ctx.map_build(xyz)
        for k in (7, 10):
            out = ctx.map_normals(capi.default_surface_params(k=k, max_dist=1.0))
            ref = sr.normals(xyz, k=k, max_dist=1.0)
            # (every lattice neighbourhood is symmetric or nearly so: the gap decides what is compared, n_used / distances are exact)
            _check_normals(out, ref, label=f"lattice k={k}")
            idx, d2, found = ctx.map_knn(xyz, k, 1.0)
            assert np.array_equal(np.where(idx == 0xFFFFFFFF, -1, idx.astype(np.int64)), ref["idx"])


def test_tiny_duplicated_and_isolated_maps(capi):
    with capi.Context() as ctx:
        two = np.array([[0, 0, 0], [0.3, 0, 0]], np.float32)
        ctx.map_build(two)
        out = ctx.map_normals(capi.default_surface_params(k=5, min_neighbours=3))
        assert list(out["n_used"]) == [2, 2] and np.all(out["normals"] == 0) and np.all(np.isnan(out["curvature"]))
        assert np.allclose(out["mean_dist"], 0.3, rtol=1e-6)
        n, flags, _ = ctx.map_remove_outliers(capi.default_outlier_params(mode=1, radius=0.5, min_neighbours=1), dry_run=True)
        assert n == 0 and list(flags) == [0, 0]
        n, flags, _ = ctx.map_remove_outliers(capi.default_outlier_params(mode=1, radius=0.5, min_neighbours=2), dry_run=True)
        assert list(flags) == [1, 1]
    rng = np.random.default_rng(5)
    base = rng.uniform(-2, 2, (3000, 3)).astype(np.float32)
    dup = np.concatenate([base, base[:1000], base[:300]])
    with capi.Context() as ctx:
        ctx.map_build(dup)
        out = ctx.map_normals(capi.default_surface_params(k=8))
        ref = sr.normals(dup, k=8)
        # A neighbourhood of coincident points has a rank-deficient covariance: l0 is 0 in exact arithmetic and rounding noise in
        # both solvers, so 2 ulp OF THE CURVATURE means nothing there.  l0 carries each solver's absolute error, 8 eps64 trace
        # (the bound tests/test_surface_host.py holds the device's solver to), so l0 / trace is known to 16 eps64 absolutely:
        # that floor comes off before the 2 ulp, here only (DESIGN.md §2 records the finding).
        _check_normals(out, ref, label="duplicates", cv_floor=16 * np.finfo(np.float64).eps)
        cnt = sr.radius_counts(dup, 0.3)
        _, flags, _ = ctx.map_remove_outliers(capi.default_outlier_params(mode=1, radius=0.3, min_neighbours=4), dry_run=True)
        assert np.array_equal(flags.astype(bool), cnt < 4)
        # max_dist so small that every point is alone (duplicates aside: take the distinct ones)
        ctx.map_build(base)
        out = ctx.map_normals(capi.default_surface_params(k=5, max_dist=1e-4))
        assert np.all(out["n_used"] == 1) and np.all(out["normals"] == 0) and np.all(np.isnan(out["curvature"]))
        assert np.all(np.isposinf(out["mean_dist"]))


def test_after_an_eviction_and_with_an_insert_in_flight(capi, scene):
    xyz = scene["map_xyz"][:40_000]
    extra = scene["map_xyz"][40_000:45_000]
    with capi.Context() as ctx:
        ctx.map_build(xyz)
        ctx.map_evict_box(np.array([-1e3, -1e3, -1e3], np.float32), np.array([1e3, 0.0, 1e3], np.float32), keep_inside=False)
        left = ctx.map_fetch()
        assert 0 < len(left) < len(xyz)
        out = ctx.map_normals()
        _check_normals(out, sr.normals(left), label="evicted")
        ctx.map_add(extra)   # (the insert runs beside the caller: the next call settles it)
        out = ctx.map_normals()
        now = ctx.map_fetch()
        assert len(now) == len(left) + len(extra)
        _check_normals(out, sr.normals(now), label="insert in flight")


def _with_ghosts(scene, ghosts):
    xyz = np.concatenate([scene["map_xyz"], ghosts])
    return xyz[np.random.default_rng(9).permutation(len(xyz))]


def test_outliers_dry_run(capi, scene, ghosts):
    xyz = _with_ghosts(scene, ghosts)
    is_ghost = np.zeros(len(xyz), bool)
    tree = cKDTree(ghosts.astype(np.float64))
    is_ghost[tree.query(xyz.astype(np.float64))[0] == 0] = True
    assert is_ghost.sum() == len(ghosts)
    with capi.Context() as ctx:
        ctx.map_build(xyz)
        n, flags, _ = ctx.map_remove_outliers(capi.default_outlier_params(mode=1, radius=0.5, min_neighbours=3), dry_run=True)
        ref1 = sr.outliers_radius(xyz, 0.5, 3)
        assert n == 0 and np.array_equal(flags.astype(bool), ref1) and np.all(flags[is_ghost] == 1)
        n, flags, stats = ctx.map_remove_outliers(capi.default_outlier_params(mode=0, k=10, std_mul=2.0, max_dist=2.0), dry_run=True)
        assert ctx.map_size() == len(xyz)
    ref0, d, st = sr.outliers_statistical(xyz, 10, 2.0, 2.0)
    rel = np.abs(stats - np.array(st)) / np.abs(np.array(st))
    band = np.abs(d - st[2]) <= 1e-9
    print("stats", stats, "reference", st, "relative error", rel, "in band", int(band.sum()), "flagged", int(flags.sum()))
    assert n == 0 and np.all(rel <= 1e-9), rel
    assert np.array_equal(flags.astype(bool)[~band], ref0[~band])
    assert band.sum() <= 1e-3 * len(xyz)
    # every ghost is flagged: its nearest other point is >= 1 m away, so its d is +inf or >= 1 m, far above the threshold
    assert np.all(flags[is_ghost] == 1) and np.all(d[is_ghost] >= 1.0)


@pytest.mark.parametrize("mode", [0, 1])
def test_outlier_removal_end_to_end(capi, scene, ghosts, mode):
    xyz = _with_ghosts(scene, ghosts)
    prm = capi.default_outlier_params(mode=mode, k=10, std_mul=2.0, max_dist=2.0, radius=0.5, min_neighbours=3)
    if mode == 0:
        ref, d, st = sr.outliers_statistical(xyz, 10, 2.0, 2.0)
        band = np.abs(d - st[2]) <= 1e-9   # (may go either way: test_outliers_dry_run)
    else:
        ref, band = sr.outliers_radius(xyz, 0.5, 3), np.zeros(len(xyz), bool)
    with capi.Context() as ctx:
        ctx.map_build(xyz)
        _, dry, _ = ctx.map_remove_outliers(prm, dry_run=True)
        n, flags, _ = ctx.map_remove_outliers(prm)
        assert n == int(dry.sum()) and np.array_equal(flags, dry)
        assert np.array_equal(dry.astype(bool)[~band], ref[~band]) and band.sum() <= 1e-3 * len(xyz)
        # the reference's survivors (inside the band, where there is any, the device's own decision)
        keep = xyz[np.where(band, dry == 0, ~ref)]
        assert ctx.map_size() == len(keep)
        assert np.array_equal(_bits(ctx.map_fetch()), _bits(keep))
        q = keep[::97]
        idx, d2, found = ctx.map_knn(q, 5)
        ridx, rd2, _ = _knn_of(keep, q, 5)
        assert np.array_equal(idx.astype(np.int64), ridx) and np.array_equal(_bits(d2), _bits(rd2))
        ctx.map_add(scene["map_xyz"][:2000] + np.float32(0.013))
        assert ctx.map_size() == len(keep) + 2000
        ctx.scan_set(scene["scan_xyz"])
        x, P, passes, _, _ = ctx.update(scene["x_init"], scene["P0"])
    with capi.Context() as ctx:   # the map without ghosts
        ctx.map_build(scene["map_xyz"])
        ctx.scan_set(scene["scan_xyz"])
        x0, _, passes0, _, _ = ctx.update(scene["x_init"], scene["P0"])
    e, e0 = np.linalg.norm(x[:3] - scene["x_true"][:3]), np.linalg.norm(x0[:3] - scene["x_true"][:3])
    print(f"mode {mode}: removed {n}, position error {e:.2e} m in {passes} passes; without ghosts {e0:.2e} m in {passes0}")
    # x_init is 0.13 m off; 4000 scan points of sigma 0.01 m fix the position to ~ sigma / sqrt(n) * a few: both within 5 mm
    assert e <= 5e-3 and e0 <= 5e-3


def _knn_of(cloud, q, k):
    """(idx, d2, found) of arbitrary queries against a cloud, (d2 f32, index) order."""
    tree = cKDTree(cloud.astype(np.float64))
    _, ii = tree.query(q.astype(np.float64), k=k + 8)
    d = sr.calc_dist(q[:, None, :], cloud[ii])
    key = np.sort((d.view(np.uint32).astype(np.uint64) << np.uint64(32)) | ii.astype(np.uint64), axis=1)[:, :k]
    return (key & np.uint64(0xFFFFFFFF)).astype(np.int64), (key >> np.uint64(32)).astype(np.uint32).view(np.float32), None


def test_removal_right_after_an_insert_sees_it(capi, scene, ghosts):
    with capi.Context() as ctx:
        ctx.map_build(scene["map_xyz"][:50_000])
        ctx.map_add(ghosts)
        n, flags, _ = ctx.map_remove_outliers(capi.default_outlier_params(mode=1, radius=0.5, min_neighbours=1))
        assert len(flags) == 50_000 + len(ghosts) and np.all(flags[50_000:] == 1) and n == int(flags.sum())
        assert ctx.map_size() == 50_000 + len(ghosts) - n


def test_removal_during_a_background_rebuild(capi, scene, ghosts):
    xyz = _with_ghosts(scene, ghosts)[:60_000]

    def run(ctx, background):
        ctx.set_option("async_relinearise", 1 if background else 0)
        ctx.map_build(xyz)
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
        ctx.map_add(ghosts[:100] + np.float32(0.02))
        n0 = ctx.map_remove_outliers(capi.default_outlier_params(mode=0, k=8, std_mul=1.5))[0]
        journaled = max(journaled, ctx.map_rebuild_status()["journal"])
        n1 = ctx.map_remove_outliers(capi.default_outlier_params(mode=1, radius=0.4, min_neighbours=4))[0]
        journaled = max(journaled, ctx.map_rebuild_status()["journal"])
        st = ctx.map_rebuild_status(wait=True)
        return ctx.map_fetch(), st, journaled, (n0, n1)

    with capi.Context() as a:
        fa, sa, ja, na = run(a, True)
    with capi.Context() as b:
        fb, _, _, nb = run(b, False)
    assert sa["adopted"] >= 1 and sa["state"] == 0 and ja >= 1, (sa, ja)
    assert na == nb and na[0] > 0 and na[1] > 0
    assert np.array_equal(_bits(fa), _bits(fb))


def test_invalid_arguments_change_nothing(capi, scene):
    xyz = scene["map_xyz"][:20_000]
    lib = capi.load_library()
    nan, inf = float("nan"), float("inf")
    bad_s = [dict(k=1), dict(k=33), dict(max_dist=0.0), dict(max_dist=-1.0), dict(max_dist=inf), dict(max_dist=nan), dict(min_neighbours=2),
             dict(k=6, min_neighbours=7), dict(orient=2), dict(orient=-1), dict(viewpoint=(nan, 0, 0)), dict(viewpoint=(0, inf, 0))]
    bad_o = [dict(mode=2), dict(mode=-1), dict(k=0), dict(k=32), dict(max_dist=0.0), dict(max_dist=nan), dict(std_mul=nan), dict(std_mul=inf),
             dict(mode=1, radius=0.0), dict(mode=1, radius=nan), dict(mode=1, radius=inf), dict(mode=1, min_neighbours=0)]
    with capi.Context() as ctx:
        ctx.map_build(xyz)
        probe = ctx.map_knn(xyz[::50], 5)
        m = len(xyz)
        buf = np.full(3 * m, 7.0, np.float32)
        fl = np.full(m, 9, np.uint8)
        nr = C.c_size_t(123)
        for kw in bad_s:
            p = capi.default_surface_params(**kw)
            assert lib.lv_map_normals(ctx.h, C.byref(p), buf.ctypes.data_as(C.POINTER(C.c_float)), None, None, None, m) == LV_EINVAL, kw
        assert lib.lv_map_normals(ctx.h, None, buf.ctypes.data_as(C.POINTER(C.c_float)), None, None, None, m) == LV_EINVAL
        for kw in bad_o:
            p = capi.default_outlier_params(**kw)
            assert lib.lv_map_remove_outliers(ctx.h, C.byref(p), fl.ctypes.data_as(C.POINTER(C.c_uint8)), C.byref(nr), None) == LV_EINVAL, kw
            assert nr.value == 123   # (nothing written)
        assert lib.lv_map_remove_outliers(ctx.h, None, fl.ctypes.data_as(C.POINTER(C.c_uint8)), None, None) == LV_EINVAL
        assert np.all(buf == 7.0) and np.all(fl == 9)
        assert ctx.map_size() == m
        after = ctx.map_knn(xyz[::50], 5)
        assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(probe, after))


def test_a_million_points(capi):
    from limo_velo_amd import synth

    xyz = synth.make_scene(1_000_000, 1000)["map_xyz"]
    with capi.Context() as ctx:
        ctx.map_build(xyz)
        t0 = time.perf_counter()
        out = ctx.map_normals()
        dt = time.perf_counter() - t0
    # (there is one launch, the ladder, for every point: the share it finishes is 1 by construction; DESIGN.md §2 has the share a
    # level-0 launch left over when one was tried, 0.17 % at this k)
    print(f"1 M points: {dt * 1e3:.1f} ms (first call), share of points finished by the ladder launch 1.0")
    pick = np.sort(np.random.default_rng(1).choice(len(xyz), 2000, replace=False))
    # the reference of the sampled points: their neighbourhoods searched in the whole cloud
    idx, d2, _ = _knn_of(xyz, xyz[pick], 10)
    sub = np.concatenate([xyz[pick], xyz[np.setdiff1d(np.unique(idx), pick)]])
    # (ids change in the sub-cloud, so ties may order differently: compare what does not depend on the order of equal distances)
    ref = sr.normals(sub, k=10)
    sel = np.zeros(len(sub), bool)
    sel[:len(pick)] = True
    got = {key: np.concatenate([out[key][pick], np.zeros((len(sub) - len(pick),) + out[key].shape[1:], out[key].dtype)]) for key in out}
    share = _check_normals(got, ref, sel=sel, label="1 M sample")
    assert share <= 0.01
