"""lv_surf_sample and lv_surf_align (include/limovelo_hip.h "Surface registration") on the GPU, through capi, against
tests/surf_align_ref.py on the scenes of tests/surf_align_cases.py: a volume of 48 x 40 x 32 voxels, 513 source points, five
guesses; nothing larger.

The sample is held by equality: only + - * / and floor occur, in f64, in one order, and the library is built without
contraction.  The alignment is held by the bounds of tests/test_gpu_ndt.py, the project's own for this kind of solve: counts and
status by equality, a pose distance of 1e-8, cost and info at 1e-9 relative.  The reference with its sums reversed ends at most
1e-11 from itself on these cases (tests/test_surf_align_ref.py), so the bounds cover the device's tree sums and its sin, cos and
sqrt many times over."""
import ctypes as C

import numpy as np
import pytest

import surf_align_cases as cases
import surf_align_ref as sr

pytestmark = pytest.mark.gpu

F = np.float32
LV_OK, LV_EINVAL, LV_ESTATE = 0, -1, -4


@pytest.fixture(scope="module")
def capi(lv):
    from limo_velo_amd import capi as c

    return c


def _load(capi, ctx, vol, params=None):
    ctx.tsdf_configure(capi.default_tsdf_params(**dict(cases.PARAMS if params is None else params)))
    ctx.tsdf_load(vol["S"], vol["W"])


@pytest.fixture(scope="module")
def ctx(capi):
    """one context with the room corner loaded; a test that loads another volume puts the corner back"""
    with capi.Context() as c:
        _load(capi, c, cases.volume())
        yield c


def _same_sample(ctx, vol, pts, min_weight=1):
    d, n, status = ctx.surf_sample(pts, min_weight)
    rd, rn, rs = sr.sample(vol, np.asarray(pts, F).astype(np.float64), min_weight)
    assert d.dtype == np.float64 and n.shape == (len(pts), 3) and status.dtype == np.uint8
    assert np.array_equal(status, rs)
    assert d.tobytes() == rd.tobytes() and n.tobytes() == rn.tobytes()       # every bit
    return status


# ---- the sample
def test_sample_against_reference(ctx, capi):
    pts = cases.sample_points(np.random.default_rng(2))
    assert len(pts) == 4096
    status = _same_sample(ctx, cases.volume(), pts)
    assert (np.bincount(status, minlength=3) >= 300).all()                   # inside the band, next to W = 0, outside, NaN and inf
    d, n, status = ctx.surf_sample(np.zeros((0, 3), F))                      # n = 0
    assert len(d) == 0 and n.shape == (0, 3) and len(status) == 0
    x, _, _ = sr.transform(cases.source(), cases.guesses()[2])
    _same_sample(ctx, cases.volume(), x.astype(F))
    # status alone, and the values alone
    lib = capi.load_library()
    a = np.ascontiguousarray(pts[:100])
    st, out = np.full(100, 9, np.uint8), np.full(400, 7.0)
    assert lib.lv_surf_sample(ctx.h, 1, C.c_void_p(a.ctypes.data), 12, 100, None, st.ctypes.data_as(C.POINTER(C.c_uint8))) == LV_OK
    assert lib.lv_surf_sample(ctx.h, 1, C.c_void_p(a.ctypes.data), 12, 100, out.ctypes.data_as(C.POINTER(C.c_double)), None) == LV_OK
    rd, rn, rs = sr.sample(cases.volume(), a.astype(np.float64))
    assert np.array_equal(st, rs) and np.array_equal(out.reshape(100, 4), np.concatenate([rd[:, None], rn], axis=1))


def test_sample_with_min_weight_and_on_cell_faces(ctx, capi):
    pts = cases.sample_points(np.random.default_rng(2))
    _load(capi, ctx, cases.volume(True))
    s1 = _same_sample(ctx, cases.volume(True), pts, 1)
    s3 = _same_sample(ctx, cases.volume(True), pts, 3)
    assert ((s1 == sr.KNOWN) & (s3 == sr.UNKNOWN)).sum() >= 100
    # a grid in binary fractions: f = 0 exactly, i = 0 and i = n - 2, and the field comes back as it is
    _load(capi, ctx, cases.linear_volume(), cases.LINEAR)
    exact, u = cases.exact_points(np.random.default_rng(1), 1000)
    status = _same_sample(ctx, cases.linear_volume(), exact)
    assert np.all(status == sr.KNOWN) and (u == np.floor(u)).all(axis=1).sum() >= 250
    d, n, _ = ctx.surf_sample(exact)
    assert np.array_equal(d, (u @ np.array(cases.LINEAR_COEF, float) + cases.LINEAR_OFFSET) * (cases.LINEAR["resolution"] / 256.0))
    _load(capi, ctx, cases.volume())


def test_sample_after_recentre(ctx, capi):
    """lv_volume_recentre by (3, -2, 1): the reference is given the shifted volume and the shifted origin"""
    vol = cases.volume()
    shift = (3, -2, 1)
    nz, ny, nx = vol["S"].shape
    moved = {}
    for k in ("S", "W"):
        new = np.zeros_like(vol[k])
        src = vol[k][max(shift[2], 0):nz + min(shift[2], 0), max(shift[1], 0):ny + min(shift[1], 0), max(shift[0], 0):nx + min(shift[0], 0)]
        new[max(-shift[2], 0):nz + min(-shift[2], 0), max(-shift[1], 0):ny + min(-shift[1], 0), max(-shift[0], 0):nx + min(-shift[0], 0)] = src
        moved[k] = new
    origin = tuple(float(F(o) + F(s) * F(vol["resolution"])) for o, s in zip(vol["origin"], shift))
    ctx.volume_recentre(capi.LV_VOLUME_SURFACE, shift)
    try:
        got = ctx.tsdf_fetch()
        assert np.array_equal(got["S"], moved["S"]) and np.array_equal(got["W"], moved["W"]) and tuple(ctx.tsdf_params().origin) == origin
        pts = cases.sample_points(np.random.default_rng(2))
        status = _same_sample(ctx, dict(vol, origin=origin, **moved), pts)
        assert (status == sr.KNOWN).sum() >= 300
        was = sr.sample(vol, pts.astype(np.float64))
        both = (status == sr.KNOWN) & (was[2] == sr.KNOWN)
        d, _, _ = ctx.surf_sample(pts)
        assert both.sum() >= 300 and np.abs(d[both] - was[0][both]).max() <= 1e-6     # the same world point, the same distance (the origin is f32)
    finally:
        _load(capi, ctx, cases.volume())


# ---- the alignment
def _compare(got, ref, k_ref=None):
    """tests/test_gpu_ndt.py's _compare with cost for score"""
    for k, g in enumerate(got):
        r = ref[k if k_ref is None else k_ref]
        assert (int(g["n_in"]), int(g["status"]), int(g["accepted"]), int(g["rejected"])) == (r["n_in"], r["status"], r["accepted"], r["rejected"]), \
            (k, g["n_in"], g["status"], g["accepted"], g["rejected"], r)
        pose = np.concatenate([g["t"], g["q"]])
        if r["status"] == sr.NO_OVERLAP:
            assert np.array_equal(pose, r["pose"]) and g["cost"] == 0.0 and not g["info"].any() and g["lambda"] == r["lambda"]
            continue
        d = sr.pose_distance(pose, r["pose"])
        rel = abs(g["cost"] - r["cost"]) / r["cost"]
        ie = np.abs(g["info"] - r["info"]).max() / np.abs(r["info"]).max()
        print("  guess", k, "distance", d, "cost rel", rel, "info rel", ie)
        assert d <= 1e-8 and rel <= 1e-9 and ie <= 1e-9
        assert g["lambda"] == pytest.approx(r["lambda"], rel=1e-12) and g["last_step"] == pytest.approx(r["last_step"], rel=1e-5, abs=1e-12)


@pytest.mark.parametrize("name", list(cases.CASES))
def test_align_against_reference(ctx, capi, name):
    c = cases.CASES[name]()
    ref, _ = cases.reference(name)
    _load(capi, ctx, c["vol"])
    try:
        res, b = ctx.surf_align(c["source"], c["guesses"], **c["solve"])
        print(name, "K =", len(c["guesses"]))
        _compare(res, ref)
        cases.check_best(b, res, name)
        # every guess alone: the reference again, and the batch's bits
        for k, g in enumerate(c["guesses"]):
            one, b1 = ctx.surf_align(c["source"], g, **c["solve"])
            assert one[0].tobytes() == res[k].tobytes()
            assert b1 == ((0, ref[k]["n_in"]) if ref[k]["status"] != sr.NO_OVERLAP else (-1, -1))
        again, b2 = ctx.surf_align(c["source"], c["guesses"], **c["solve"])
        assert again.tobytes() == res.tobytes() and b2 == b       # two runs repeat their bits
        if name == "floor":
            guess_cost = ctx.surf_align(c["source"], c["guesses"], **dict(c["solve"], max_iterations=0))[0]["cost"]
            assert np.all(res["cost"] <= guess_cost) and np.all(np.linalg.norm(res["t"] - c["guesses"][:, :3], axis=1) <= 0.2)
    finally:
        _load(capi, ctx, cases.volume())


def test_sizes_around_the_chunk(ctx, capi):
    c = cases.corner()
    vol, s = c["vol"], c["solve"]
    assert capi.SURF_ALIGN_CHUNK == sr.CHUNK
    src = cases.to_frame(cases.TRUTH, np.concatenate(cases.plane_points(np.random.default_rng(21), 171))).astype(F)
    src = src[np.random.default_rng(22).permutation(len(src))]
    assert len(src) == capi.SURF_ALIGN_CHUNK + 1
    g = c["guesses"][1:3]
    for n in (1, capi.SURF_ALIGN_CHUNK - 1, capi.SURF_ALIGN_CHUNK, capi.SURF_ALIGN_CHUNK + 1):
        res, best = ctx.surf_align(src[:n], g, **dict(s, max_iterations=0, min_points=1))
        want = []
        for k in range(2):
            acc, n_in = sr.evaluate(vol, src[:n], g[k], 1, s["max_dist"], s["huber"])
            cost = sr.cost_of(acc[27], n, n_in, s["max_dist"], s["huber"])
            want.append((cost, n_in))
            if n_in == 0:      # (one point, and it is not IN)
                assert res[k]["status"] == capi.SURF_ALIGN_NO_OVERLAP
                continue
            assert (res[k]["n_in"], res[k]["status"], res[k]["accepted"], res[k]["rejected"]) == (n_in, capi.SURF_ALIGN_MAX_ITERATIONS, 0, 0)
            assert np.array_equal(np.concatenate([res[k]["t"], res[k]["q"]]), g[k])
            assert abs(res[k]["cost"] - cost) <= 1e-9 * cost and np.abs(res[k]["info"] - acc[:21]).max() <= 1e-9 * np.abs(acc[:21]).max(), n
        live = [k for k in range(2) if want[k][1] > 0]
        kb = min(live, key=lambda k: want[k][0]) if live else -1
        assert best == ((kb, want[kb][1]) if live else (-1, -1))
    # two chunks through the whole loop
    ref = sr.align_one(vol, src, g[0], **s)
    res, _ = ctx.surf_align(src, g[:1], **s)
    _compare(res, [ref])
    assert ref["status"] == sr.CONVERGED
    res, best = ctx.surf_align(np.zeros((0, 3), F), g, **s)        # no source point: NO_OVERLAP, the poses untouched
    assert best == (-1, -1) and list(res["status"]) == [capi.SURF_ALIGN_NO_OVERLAP] * 2 and np.array_equal(np.concatenate([res["t"], res["q"]], axis=1), g)
    res, best = ctx.surf_align(src, np.zeros((0, 7)), **s)         # K = 0
    assert len(res) == 0 and best == (-1, -1)


def test_no_overlap_returns_the_guess(ctx, capi):
    c = cases.corner()
    far = c["guesses"][4]
    odd = np.array([1e30, 0, 0, 0, 0, 0, 1.0])
    g = np.stack([far, odd, c["guesses"][1]])
    res, best = ctx.surf_align(c["source"], g, **c["solve"])
    for k in (0, 1):
        r = res[k]
        assert np.concatenate([r["t"], r["q"]]).tobytes() == g[k].tobytes()
        assert (r["n_in"], r["status"], r["cost"], r["accepted"], r["rejected"], r["last_step"]) == (0, capi.SURF_ALIGN_NO_OVERLAP, 0.0, 0, 0, 0.0)
        assert not r["info"].any()
    assert res[2]["status"] == capi.SURF_ALIGN_CONVERGED and best == (2, int(res[2]["n_in"]))
    res, best = ctx.surf_align(c["source"], g[:2], **c["solve"])
    assert best == (-1, -1) and list(res["status"]) == [capi.SURF_ALIGN_NO_OVERLAP] * 2
    # fewer points IN than min_points: NO_OVERLAP too
    n_in = int(ctx.surf_align(c["source"], g[2:], **dict(c["solve"], max_iterations=0))[0][0]["n_in"])
    res, best = ctx.surf_align(c["source"], g[2:], **dict(c["solve"], min_points=n_in + 1))
    assert res[0]["status"] == capi.SURF_ALIGN_NO_OVERLAP and best == (-1, -1)
    res, best = ctx.surf_align(c["source"], g[2:], **dict(c["solve"], min_points=n_in, max_iterations=0))
    assert res[0]["status"] == capi.SURF_ALIGN_MAX_ITERATIONS and best == (0, n_in)


def test_the_calls_change_nothing(capi):
    c = cases.corner()
    rng = np.random.default_rng(9)
    wc = rng.integers(0, 4, c["vol"]["S"].shape + (1,)).astype(np.uint32)
    layer = np.concatenate([(rng.integers(0, 256, c["vol"]["S"].shape + (3,)) * wc).astype(np.uint32), wc], axis=-1)
    frm = np.tile(np.array([[1.0, 0.8, 0.4]], F), (64, 1))
    to = (frm + 1.3 * (np.concatenate(cases.plane_points(rng, 22))[:64] - frm)).astype(F)      # through the planes
    with capi.Context() as ctx:
        _load(capi, ctx, c["vol"])
        ctx.colour_load(layer)
        ctx.tsdf_mesh_build(1)

        def snapshot():
            info = ctx.tsdf_mesh_info()
            rays = ctx.tsdf_raycast(frm, to, None, True, True)
            return (ctx.tsdf_fetch(), ctx.colour_fetch()["sums"], ctx.tsdf_mesh_fetch(), (info.built, info.stale, info.vertices, info.triangles),
                    tuple(ctx.volume_shift_info().surface), [r.tobytes() for r in rays])

        def unchanged(a, b):
            assert all(np.array_equal(a[0][k], b[0][k]) for k in a[0]) and np.array_equal(a[1], b[1])
            assert all(np.array_equal(a[2][k], b[2][k]) for k in a[2]) and a[3:] == b[3:]

        before = snapshot()
        assert before[3][:2] == (1, 0) and (np.frombuffer(before[5][0], capi.TSDF_RAY_RESULT_DTYPE)["status"] == capi.LV_SURF_HIT).sum() >= 32
        res, _ = ctx.surf_align(c["source"], c["guesses"], **c["solve"])
        ctx.surf_sample(cases.sample_points(rng, 512))
        ctx.surf_sample(cases.sample_points(rng, 512), 3)
        unchanged(before, snapshot())
        ctx.colour_clear()                      # a stale mesh stays stale
        stale = snapshot()
        assert stale[3][:2] == (1, 1)
        assert ctx.surf_align(c["source"], c["guesses"], **c["solve"])[0].tobytes() == res.tobytes()
        unchanged(stale, snapshot())


def test_states(capi):
    c = cases.corner()
    lib = capi.load_library()
    src = np.ascontiguousarray(c["source"])
    g = np.ascontiguousarray(c["guesses"])
    with capi.Context() as ctx:
        def estate(call):
            with pytest.raises(capi.LvError, match="error -4.*lv_tsdf_configure first"):
                call()

        estate(lambda: ctx.surf_sample(src))
        estate(lambda: ctx.surf_sample(np.zeros((0, 3), F)))
        estate(lambda: ctx.surf_align(src, g))
        estate(lambda: ctx.surf_align(src, np.zeros((0, 7))))
        # a refused call writes nothing
        res, best = (capi.SurfAlignResult * 5)(), (C.c_int32 * 2)(7, 7)
        G = g.ctypes.data_as(C.POINTER(capi.GraphPose))
        assert lib.lv_surf_align(ctx.h, None, C.c_void_p(src.ctypes.data), 12, len(src), G, 5, res, best) == LV_ESTATE
        assert list(best) == [7, 7] and not bytes(res).strip(b"\0")
        _load(capi, ctx, c["vol"])
        bad = capi.default_surf_align_params(max_dist=0.0)
        assert lib.lv_surf_align(ctx.h, C.byref(bad), C.c_void_p(src.ctypes.data), 12, len(src), G, 5, res, best) == LV_EINVAL
        assert lib.lv_surf_align(ctx.h, None, C.c_void_p(src.ctypes.data), 8, len(src), G, 5, res, best) == LV_EINVAL
        assert list(best) == [7, 7] and not bytes(res).strip(b"\0")
        out, st = np.full(8, 7.0), np.full(2, 9, np.uint8)
        assert lib.lv_surf_sample(ctx.h, 0, C.c_void_p(src.ctypes.data), 12, 2, out.ctypes.data_as(C.POINTER(C.c_double)),
                                  st.ctypes.data_as(C.POINTER(C.c_uint8))) == LV_EINVAL
        assert np.all(out == 7.0) and np.all(st == 9)
        with pytest.raises(capi.LvError, match="error -1.*huber"):
            ctx.surf_align(src, g, huber=-1.0)
        good, b = ctx.surf_align(src, g, **c["solve"])
        assert b[0] in range(4)
        # a reconfigure without a load: an all-unknown volume, every guess NO_OVERLAP, every point UNKNOWN or OUTSIDE
        ctx.tsdf_configure(capi.default_tsdf_params(**cases.PARAMS))
        res2, b2 = ctx.surf_align(src, g, **c["solve"])
        assert b2 == (-1, -1) and list(res2["status"]) == [capi.SURF_ALIGN_NO_OVERLAP] * 5
        assert np.array_equal(np.concatenate([res2["t"], res2["q"]], axis=1), g)
        d, n, status = ctx.surf_sample(cases.sample_points(np.random.default_rng(2), 512))
        assert not d.any() and not n.any() and set(status.tolist()) == {sr.OUTSIDE, sr.UNKNOWN}
        _load(capi, ctx, c["vol"])                # the scratch was freed with the volume and comes back
        assert ctx.surf_align(src, g, **c["solve"])[0].tobytes() == good.tobytes()


# ---- end to end
def test_track_a_depth_camera(capi):
    """Eight frames rendered from the corner volume are fused into a fresh volume of the same box; a ninth is tracked against it
    from a guess 0.08 m and 0.05 rad off.  How near the truth it gets depends on the projective 1 / cos bias of the depth fusion:
    the error is printed, the two inequalities are asserted.  (On the numpy references of the ray caster, the fusion and this
    rule: 0.080 m -> 0.021 m and 0.050 rad -> 0.0091 rad, cost 1.159 -> 0.370, 12 accepted and 19 rejected steps.)"""
    from limo_velo_amd import mesh

    cam = cases.CAMERA
    poses = cases.track_poses()
    with capi.Context() as room, capi.Context() as ctx:
        _load(capi, room, cases.volume())
        frames = [mesh.render_frame(room, R, t, cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["width"], cam["height"], cases.TRACK_RANGE) for R, t in poses]
        assert all(np.isfinite(f["depth"]).mean() > 0.9 for f in frames)
        ctx.tsdf_configure(capi.default_tsdf_params(**cases.PARAMS))
        stats = mesh.integrate_depth(ctx, frames[:8])
        assert stats[3] > 3000
        last = frames[8]
        guess = cases.track_guess(last["R"], last["t"])
        pts = mesh.frame_points(last, 4)
        g = np.concatenate([guess[1], mesh._quat_of(guess[0])])
        at_guess, _ = mesh.align(ctx, pts, g, max_iterations=0)
        R, t, res = mesh.track_depth(ctx, last, guess, stride=4)
        e0 = (float(np.linalg.norm(guess[1] - last["t"])), cases.rotation_angle(guess[0], last["R"]))
        e1 = (float(np.linalg.norm(t - last["t"])), cases.rotation_angle(R, last["R"]))
        print("track_depth:", len(pts), "points, n_in", int(at_guess[0]["n_in"]), "->", int(res["n_in"]), "cost", float(at_guess[0]["cost"]), "->",
              float(res["cost"]), "translation error", e0[0], "->", e1[0], "rotation error", e0[1], "->", e1[1], "accepted", int(res["accepted"]),
              "rejected", int(res["rejected"]))
        assert res["status"] == capi.SURF_ALIGN_CONVERGED
        assert res["cost"] < at_guess[0]["cost"]
        assert e1[0] < e0[0] and e1[1] < e0[1]
        p = mesh.align_params_for(ctx)
        assert p.max_dist == 2 * float(F(0.1)) and p.huber == float(F(0.1)) / 2
