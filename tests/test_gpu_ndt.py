"""lv_ndt_* (include/limovelo_hip.h "NDT registration") on the GPU, through capi, against tests/ndt_ref.py on the scenes of
tests/ndt_cases.py: 4000 target and 400 source points over 8 x 8 x 4 voxels, nothing larger.

The moments are integer sums and are held by equality.  MEAN and COV are held at 1e-12 relative, Sigma Omega = I at 1e-9 (the
condition number is at most 3 / reg + 1 = 301).  The alignment is held at a pose distance of 1e-8: the reference run with its
sums reversed ends at most 4.4e-16 from itself on these cases (tests/test_ndt_ref.py), so 1e-8 covers the device's exp and its
tree sums many times over; score and info at 1e-9 relative; n_in, status and the accepted and rejected counts by equality."""
import ctypes as C
import math

import numpy as np
import pytest

import graph_ref as gr
import ndt_cases as cases
import ndt_ref as nr

pytestmark = pytest.mark.gpu

LV_OK, LV_EINVAL, LV_ESTATE = 0, -1, -4
LAYERS = ("n", "S1", "S2", "mean", "cov", "icov")


@pytest.fixture(scope="module")
def capi(lv):
    from limo_velo_amd import capi as c

    return c


@pytest.fixture(scope="module")
def ctx(capi):
    with capi.Context() as c:
        yield c


def _prm(capi, p):
    return capi.default_ndt_params(**p)


def _fetch(ctx, capi):
    out = {}
    for k, name in enumerate(LAYERS):
        a = ctx.ndt_fetch(k)
        out[name] = a.reshape(-1) if capi.NDT_LAYERS[k][2] == 1 else a.reshape(-1, capi.NDT_LAYERS[k][2])
    return out


def _same_bits(a, b):
    return all(a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes() for k in LAYERS)


def _check_against_reference(got, T, min_points=5):
    for k in ("n", "S1", "S2"):
        assert got[k].dtype == T[k].dtype and np.array_equal(got[k], T[k]), k
    used = T["n"] >= min_points
    assert used.sum() > 0
    for k in ("mean", "cov"):
        assert np.abs(got[k][used] - T[k][used]).max() <= 1e-12 * np.abs(T[k][used]).max(), k
        assert np.all(np.abs(got[k][used] - T[k][used]) <= 1e-12 * np.abs(T[k][used]).max(axis=1, keepdims=True))
    for k in ("mean", "cov", "icov"):
        assert not got[k][~used].any(), k
    worst = max(np.abs(nr.full3(got["cov"][c]) @ nr.full3(got["icov"][c]) - np.eye(3)).max() for c in np.nonzero(used)[0])
    assert worst <= 1e-9, worst


# ---- the target
@pytest.mark.parametrize("name", ["corner-near", "plane"])
def test_build_against_reference(ctx, capi, name):
    c = cases.ALIGN_CASES[name]()
    T = cases.target(name)
    stats = ctx.ndt_build(_prm(capi, c["prm"]), c["target"])
    assert stats.tolist() == nr.stats(T)
    got = _fetch(ctx, capi)
    _check_against_reference(got, T)
    i = ctx.ndt_info()
    assert (i.built, i.from_map, i.n_used, i.n_ignored, i.used_voxels, i.sparse_voxels) == (1, 0, *nr.stats(T))
    assert bytes(i.params) == bytes(_prm(capi, c["prm"]))
    # the same points in another order: every layer, bit for bit
    ctx.ndt_build(_prm(capi, c["prm"]), c["target"][np.random.default_rng(2).permutation(len(c["target"]))])
    assert _same_bits(_fetch(ctx, capi), got)
    # build(a) + add(b) is build(a u b)
    ctx.ndt_build(_prm(capi, c["prm"]), c["target"][:1500])
    s2 = ctx.ndt_add(c["target"][1500:])
    assert _same_bits(_fetch(ctx, capi), got)
    ok_b = int(nr.voxel_of(c["prm"], c["target"][1500:])[0].sum())
    assert s2.tolist() == [ok_b, len(c["target"]) - 1500 - ok_b, *nr.stats(T)[2:]] and ctx.ndt_info().n_used == nr.stats(T)[0]


def test_build_edge_cases(ctx, capi):
    for prm, pts in (cases.coincident(), cases.dirty()):
        T = nr.build(prm, pts)
        assert ctx.ndt_build(_prm(capi, prm), pts).tolist() == nr.stats(T)
        _check_against_reference(_fetch(ctx, capi), T)
    assert ctx.ndt_build(_prm(capi, prm), np.zeros((0, 3), np.float32)).tolist() == [0, 0, 0, 0]
    assert not any(v.any() for v in _fetch(ctx, capi).values())


def test_build_from_the_device_map(capi):
    c = cases.corner_near()
    with capi.Context() as ctx:
        p = _prm(capi, c["prm"])
        assert ctx.ndt_build(p, None).tolist() == [0, 0, 0, 0] and ctx.ndt_info().from_map == 1     # no map yet: an empty target
        ctx.map_build(c["target"])
        gone = ctx.map_evict_box((2.5, 2.5, -1.0), (4.5, 4.5, 2.0), keep_inside=False)               # the box leaves the map
        assert gone > 100
        living = ctx.map_fetch()
        s_map = ctx.ndt_build(p, None)
        from_map = _fetch(ctx, capi)
        assert ctx.ndt_info().from_map == 1
        s_pts = ctx.ndt_build(p, living)
        assert s_map.tolist() == s_pts.tolist() == nr.stats(nr.build(c["prm"], living)) and _same_bits(_fetch(ctx, capi), from_map)
        assert np.array_equal(ctx.map_fetch().view(np.uint32), living.view(np.uint32))
        ctx.ndt_build(p, living[:1000])
        ctx.ndt_add(None)
        both = nr.build(c["prm"], np.concatenate([living[:1000], living]))
        assert np.array_equal(_fetch(ctx, capi)["S2"], both["S2"])


# ---- the alignment
def _compare(got, ref, k_ref=None):
    for k, g in enumerate(got):
        r = ref[k if k_ref is None else k_ref]
        assert (int(g["n_in"]), int(g["status"]), int(g["accepted"]), int(g["rejected"])) == (r["n_in"], r["status"], r["accepted"], r["rejected"]), \
            (k, g["n_in"], g["status"], g["accepted"], g["rejected"], r)
        pose = np.concatenate([g["t"], g["q"]])
        d = nr.pose_distance(pose, r["pose"])
        rel = abs(g["score"] - r["score"]) / r["score"]
        ie = np.abs(g["info"] - r["info"]).max() / np.abs(r["info"]).max()
        print("  guess", k, "distance", d, "score rel", rel, "info rel", ie)
        assert d <= 1e-8 and rel <= 1e-9 and ie <= 1e-9
        assert g["lambda"] == pytest.approx(r["lambda"], rel=1e-12) and g["last_step"] == pytest.approx(r["last_step"], rel=1e-5, abs=1e-12)


@pytest.fixture(scope="module")
def aligned(ctx, capi):
    """every case once, all eight guesses in one call: {name: (results, best)}"""
    out = {}
    for name, make in cases.ALIGN_CASES.items():
        c = make()
        ctx.ndt_build(_prm(capi, c["prm"]), c["target"])
        out[name] = ctx.ndt_align(c["source"], c["guesses"], **c["solve"])
    return out


@pytest.mark.parametrize("name", list(cases.ALIGN_CASES))
def test_align_against_reference(ctx, capi, aligned, name):
    c = cases.ALIGN_CASES[name]()
    ref, best = cases.reference(name)
    res, b = aligned[name]
    print(name, "K = 8")
    _compare(res, ref)
    assert b == best
    # every guess alone: the reference again, and the batch's bits
    ctx.ndt_build(_prm(capi, c["prm"]), c["target"])
    for k, g in enumerate(c["guesses"]):
        one, b1 = ctx.ndt_align(c["source"], g, **c["solve"])
        _compare(one, ref, k)
        assert one[0].tobytes() == res[k].tobytes() and b1 == (0, ref[k]["n_in"])
    again, b2 = ctx.ndt_align(c["source"], c["guesses"], **c["solve"])
    assert again.tobytes() == res.tobytes() and b2 == b       # two runs repeat their bits


def test_scores_only_and_no_overlap(ctx, capi):
    c = cases.corner_near()
    T = cases.target("corner-near")
    ctx.ndt_build(_prm(capi, c["prm"]), c["target"])
    far = np.array([500.0, 0, 0, 0, 0, 0, 1.0])
    odd = np.array([1e30, 0, 0, 0, 0, 0, 1.0])      # does not quantise at all
    g = np.concatenate([c["guesses"][:3], [far, odd]])
    for search in (1, 7):
        res, best = ctx.ndt_align(c["source"], g, **dict(c["solve"], max_iterations=0, search=search))
        want = [nr.evaluate(c["prm"], T, c["source"], x, search, cases.D2) for x in g[:3]]
        for k, (acc, n_in) in enumerate(want):
            r = res[k]
            assert np.array_equal(np.concatenate([r["t"], r["q"]]), g[k]) and (r["n_in"], r["status"], r["accepted"], r["rejected"]) == (n_in, 1, 0, 0)
            assert abs(r["score"] - acc[27]) <= 1e-9 * acc[27] and np.abs(r["info"] - acc[:21]).max() <= 1e-9 * np.abs(acc[:21]).max()
        for k in (3, 4):
            r = res[k]
            assert np.array_equal(np.concatenate([r["t"], r["q"]]), g[k]) and (r["n_in"], r["status"], r["score"]) == (0, capi.NDT_NO_OVERLAP, 0.0)
            assert not r["info"].any()
        kb = int(np.argmax([w[0][27] for w in want]))
        assert best == (kb, want[kb][1])
    res, best = ctx.ndt_align(c["source"], [far, odd], **c["solve"])
    assert best == (-1, -1) and list(res["status"]) == [capi.NDT_NO_OVERLAP] * 2
    res, best = ctx.ndt_align(c["source"], np.zeros((0, 7)), **c["solve"])      # K = 0
    assert len(res) == 0 and best == (-1, -1)


def test_sizes_around_the_chunk(ctx, capi):
    c = cases.corner_near()
    T = cases.target("corner-near")
    ctx.ndt_build(_prm(capi, c["prm"]), c["target"])
    rng = np.random.default_rng(21)
    src = cases.to_frame(cases.TRUTH, cases.room_points(rng, capi.NDT_CHUNK + 1)).astype(np.float32)
    g = c["guesses"][:2]
    assert capi.NDT_CHUNK == nr.CHUNK
    for n in (1, capi.NDT_CHUNK - 1, capi.NDT_CHUNK, capi.NDT_CHUNK + 1):
        res, best = ctx.ndt_align(src[:n], g, **dict(c["solve"], max_iterations=0))
        for k in range(2):
            acc, n_in = nr.evaluate(c["prm"], T, src[:n], g[k], 7, cases.D2)
            assert res[k]["n_in"] == n_in and n_in >= n - 2
            assert abs(res[k]["score"] - acc[27]) <= 1e-9 * acc[27] and np.abs(res[k]["info"] - acc[:21]).max() <= 1e-9 * np.abs(acc[:21]).max(), n
    # two chunks through the whole loop
    ref = nr.align_one(c["prm"], T, src, g[0], **c["solve"])
    res, _ = ctx.ndt_align(src, g[:1], **c["solve"])
    _compare(res, [ref])
    res, best = ctx.ndt_align(np.zeros((0, 3), np.float32), g, **c["solve"])   # no source point: NO_OVERLAP, the poses untouched
    assert best == (-1, -1) and list(res["status"]) == [capi.NDT_NO_OVERLAP] * 2 and np.array_equal(np.concatenate([res["t"], res["q"]], axis=1), g)


# ---- states
def test_states(capi):
    c = cases.corner_near()
    lib = capi.load_library()
    with capi.Context() as ctx:
        p = _prm(capi, c["prm"])

        def estate(call):
            with pytest.raises(capi.LvError, match="error -4.*lv_ndt_build first"):
                call()

        for _ in range(2):      # before a build, and after clear
            assert ctx.ndt_info().built == 0
            estate(lambda: ctx.ndt_add(c["target"]))
            estate(lambda: ctx.ndt_fetch(capi.NDT_COUNT))
            estate(lambda: ctx.ndt_align(c["source"], c["guesses"][:1]))
            estate(lambda: ctx.ndt_align(c["source"], np.zeros((0, 7))))
            ctx.ndt_build(p, c["target"])
            assert ctx.ndt_info().built == 1
            ctx.ndt_clear()
        # other stores: the map, the filter and an occupancy grid are not touched by any call
        ctx.map_build(c["target"])
        x0 = np.zeros(26)
        x0[:3], x0[6], x0[10] = (1.0, 2.0, 3.0), 1.0, 1.0
        ctx.filter_set(x0, np.eye(23) * 0.01)
        ctx.occ_configure(capi.default_occupancy_params(origin=(-1.0, -1.0, -0.5), resolution=0.5, nx=16, ny=16, nz=8))
        L = np.clip(np.random.default_rng(4).normal(size=(8, 16, 16)), -2.0, 3.5).astype(np.float32)
        ctx.occ_load(L)
        before = (ctx.map_fetch().tobytes(), ctx.filter_get()[0].tobytes(), ctx.filter_get()[1].tobytes(), ctx.occ_fetch().tobytes())
        ctx.ndt_build(p, None)
        ctx.ndt_add(c["target"][:100])
        ctx.ndt_build(p, c["target"])
        held = _fetch(ctx, capi)
        res, _ = ctx.ndt_align(c["source"], c["guesses"][:2], **c["solve"])
        # refused calls leave the target as it is, bit for bit
        stats = (C.c_uint64 * 4)()
        bad = _prm(capi, dict(c["prm"], nx=0))
        a = np.ascontiguousarray(c["target"][:10])
        assert lib.lv_ndt_build(ctx.h, C.byref(bad), C.c_void_p(a.ctypes.data), 12, 10, stats) == LV_EINVAL
        assert lib.lv_ndt_build(ctx.h, C.byref(p), C.c_void_p(a.ctypes.data), 8, 10, stats) == LV_EINVAL
        assert lib.lv_ndt_add(ctx.h, C.c_void_p(a.ctypes.data), 8, 10, stats) == LV_EINVAL
        with pytest.raises(capi.LvError, match="error -1"):
            ctx.ndt_align(c["source"], c["guesses"][:2], search=3)
        out = np.zeros(8, np.uint32)
        assert lib.lv_ndt_fetch(ctx.h, 0, C.c_void_p(out.ctypes.data), 8) == LV_EINVAL and "voxels needed" in lib.lv_last_error().decode()
        assert _same_bits(_fetch(ctx, capi), held) and ctx.ndt_info().built == 1
        res2, _ = ctx.ndt_align(c["source"], c["guesses"][:2], **c["solve"])
        assert res2.tobytes() == res.tobytes()
        after = (ctx.map_fetch().tobytes(), ctx.filter_get()[0].tobytes(), ctx.filter_get()[1].tobytes(), ctx.occ_fetch().tobytes())
        assert before == after


# ---- Python
def test_register(ctx, capi):
    """ndt.register over grid_for's own grid (origin -2, -2, -2: the floor and the walls lie on voxel faces there) against the
    reference over the same grid.  The reference ends at most 3.4e-3 from the truth, measured; twice that is asserted."""
    from limo_velo_amd import ndt

    c = cases.corner_near()
    best, res, k = ndt.register(ctx, c["target"], c["source"], c["guesses"], resolution=1.0, margin=1.0, **dict(c["solve"]))
    p = ctx.ndt_info().params
    prm = dict(origin=tuple(p.origin), resolution=p.resolution, nx=p.nx, ny=p.ny, nz=p.nz, min_points=p.min_points, reg=p.reg)
    assert prm == dict(origin=(-2.0, -2.0, -2.0), resolution=1.0, nx=10, ny=9, nz=7, min_points=5, reg=0.01)
    ref, rb = nr.align(prm, nr.build(prm, c["target"]), c["source"], c["guesses"], **c["solve"])
    _compare(res, ref)
    d = [nr.pose_distance(r["pose"], cases.TRUTH) for r in ref]
    print("register: the reference's distance from the truth", d)
    assert k == rb[0] and best["score"] == res["score"].max() and max(d) <= 2 * 3.4e-3


def test_registration_closes_a_square(ctx, capi):
    """Four keyframes round the room's box, odometry with drift; the closing edge 0 -> 3 comes from registering keyframe 3's
    cloud to keyframe 0's.  The device's registration is held to the reference's, and the graph solved on the device with the
    reference's edge to the reference's dense solution at the graph test's bound of 1e-9."""
    from limo_velo_amd import graph as pg, ndt, synth

    rng = np.random.default_rng(31)
    truth = [np.concatenate([[1.5, 1.5, 1.0], gr.quat_rpy(0, 0, 0.1)]), np.concatenate([[4.8, 1.6, 1.0], gr.quat_rpy(0, 0, 1.6)]),
             np.concatenate([[4.7, 4.9, 1.0], gr.quat_rpy(0, 0, 3.0)]), np.concatenate([[1.6, 4.6, 1.0], gr.quat_rpy(0, 0, -1.5)])]
    clouds = [cases.to_frame(x, cases.room_points(rng, 4000 if k == 0 else 400)).astype(np.float32) for k, x in enumerate(truth)]
    drifted = [truth[0]]
    for k in range(1, 4):      # odometry: the true relative pose plus drift
        t, q = gr.relative(truth[k - 1], truth[k])
        drifted.append(gr.compose(drifted[-1], t + rng.normal(0, 0.04, 3), gr.qmul(q, gr.qexp(rng.normal(0, 0.01, 3)))))
    assert 0.2 < nr.pose_distance(drifted[3], truth[3]) < 0.25
    world0 = (clouds[0].astype(np.float64) @ gr.rot(truth[0][3:]).T + truth[0][:3]).astype(np.float32)
    prm = dict(cases.ROOM)
    ctx.ndt_build(_prm(capi, prm), world0)
    res, best = ctx.ndt_align(clouds[3], [drifted[3]], **cases.SOLVE)
    ref = nr.align_one(prm, nr.build(prm, world0), clouds[3], drifted[3], **cases.SOLVE)
    _compare(res, [ref])
    assert best[0] == 0 and nr.pose_distance(ref["pose"], truth[3]) <= 2 * 4.8e-3      # (measured: 4.8e-3)

    def solve(result):
        G = pg.PoseGraph()
        for x in drifted:
            G.add_keyframe(synth.make_state(x[:3], x[3:]), sigma_t=0.05, sigma_r=0.02)
        t, q, info = ndt.loop_measurement(synth.make_state(truth[0][:3], truth[0][3:]), result)
        G.add_registration(0, 3, t, q, info / np.abs(info).max() * 1e4)     # the measurement's shape at a weight above the odometry's
        G.optimise(ctx, step_tol=1e-10, max_iterations=100)
        return G

    as_record = np.zeros((), capi.NDT_RESULT_DTYPE)
    as_record["t"], as_record["q"], as_record["info"] = ref["pose"][:3], ref["pose"][3:], ref["info"]
    G = solve(as_record)
    poses, fixed, edges, priors = G.records()
    dense, _ = gr.dense_gn(gr.make_graph(poses, fixed, edges, priors))
    d = gr.distance(G.poses, dense)
    print("square: device graph against dense", d)
    assert d <= 1e-9
    Gd = solve(res[0])      # the device's own edge: the square closes
    assert gr.distance(Gd.poses, G.poses) <= 1e-6
    # the reference's graph leaves keyframe 3 at 0.024 from the truth (measured), against a drift of 0.22
    assert nr.pose_distance(Gd.poses[3], truth[3]) <= 2 * 0.0241 < nr.pose_distance(drifted[3], truth[3])
