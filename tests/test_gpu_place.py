"""GPU tests of place recognition (lv_place.hip, include/limovelo_hip.h "Place recognition") against the numpy statement of the rule
in tests/place_ref.py: scan and map descriptors bin for bin, retrieval against f64 distances, the meaning of the shift, the limits
and states of the calls, and global relocalisation without a prior in a 1 M-point scene, from keyframes and from map places."""
import math

import numpy as np
import pytest

import place_ref as pr

pytestmark = pytest.mark.gpu

LV_EINVAL, LV_ESTATE, LV_ERANGE = -1, -4, -5
# A point decides its sector through atan2f, the one step whose f32 result the device does not share with numpy bit for bit
# (within a few ulp, ~1e-6 rad).  Bins that a point within TOL_RAD of a sector edge could change are left out of the bitwise
# comparison; 1e-5 rad keeps ten times that margin and leaves out fewer bins than 1e-4 would.
TOL_RAD = 1e-5


@pytest.fixture(scope="module")
def capi(lv):
    from limo_velo_amd import capi as c

    return c


@pytest.fixture(scope="module")
def synth(lv):
    from limo_velo_amd import synth as s

    return s


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _rc(ctx, name, *args):
    return getattr(ctx.lib, name)(ctx.h, *args)


def _states(synth):
    offR = synth.quat_from_rpy(0.0, 0.0, math.radians(1.5))
    return [synth.make_state((0.0, 0.0, 0.0), (0.0, 0.0, 0.0, 1.0)),
            synth.make_state((3.0, -2.0, 1.5), synth.quat_from_rpy(math.radians(2.0), math.radians(-1.0), math.radians(30.0))),
            synth.make_state((-7.0, 4.0, 1.2), synth.quat_from_rpy(math.radians(-3.0), math.radians(1.5), math.radians(-130.0)), offR,
                             (-0.17, 0.0, -0.04))]


def _compare(got, ref, und, what):
    ok = ~und
    bad = np.nonzero(ok & (_bits(got) != _bits(ref)))
    assert len(bad[0]) == 0, (what, list(zip(*bad))[:5], got[bad][:5], ref[bad][:5])
    return int(und.sum()), und.size


def test_describe_matches_the_rule(capi, synth):
    sc = synth.make_scene(200_000, 30_000)
    rects = synth.scene_surfaces(1_000_000)
    # (a sensor in free space: (3, -2) lies inside one of the scene's boxes)
    sweep = synth.ring_sweep(rects, synth.quat_to_rot(synth.quat_from_rpy(0.02, -0.01, 0.7)), np.array([-20.0, 15.0, 1.5]), 64, 1024)
    excluded = total = 0
    with capi.Context() as ctx:
        for scan in (sc["scan_xyz"], sweep):
            ctx.scan_set(scan)
            for x in _states(synth):
                got = ctx.place_describe(x)
                ref, und = pr.describe(pr.scan_q(scan, x), tol_rad=TOL_RAD)
                assert (ref > 0).sum() > 100
                e, t = _compare(got, ref, und, "describe")
                excluded += e
                total += t
    assert excluded < 0.005 * total, (excluded, total)


def test_add_map_matches_the_rule(capi, synth):
    sc = synth.make_scene(200_000, 1_000)
    L = sc["L"]
    rng = np.random.default_rng(11)
    centres = np.column_stack([rng.uniform(-L, L, 40), rng.uniform(-L, L, 40), rng.uniform(0.5, 3.0, 40)])
    edge = np.array([[L - 0.3, 0.0, 1.5], [-L + 0.2, L - 0.1, 1.5], [0.0, -L, 2.0], [L, L, 1.0], [-L - 5.0, 3.0, 1.5],
                     [10.0, L + 20.0, 1.5], [-L, -L, 0.0], [L - 1.0, -L + 1.0, 4.0], [0.0, 0.0, 9.5]])
    centres = np.concatenate([centres, edge, [[5000.0, 5000.0, 0.0]]])
    excluded = total = 0
    with capi.Context() as ctx:
        ctx.map_build(sc["map_xyz"])
        first = ctx.place_add_map(centres)
        assert first == 0 and ctx.place_count() == len(centres)
        desc, cen = ctx.place_fetch()
    assert np.array_equal(cen, centres)
    for i, c in enumerate(centres):
        ref, und = pr.describe(pr.map_q(sc["map_xyz"], c), tol_rad=TOL_RAD)
        e, t = _compare(desc[i], ref, und, f"centre {i}")
        excluded += e
        total += t
    assert not desc[-1].any(), "a centre far outside the map has an empty descriptor"
    assert excluded < 0.005 * total, (excluded, total)


def _random_places(rng, n, R=20, S=60):
    d = rng.uniform(0.0, 9.0, (n, R, S)).astype(np.float32)
    d *= rng.uniform(size=(n, 1, S)) > 0.25          # empty columns
    d *= rng.uniform(size=(n, R, S)) > 0.4           # empty bins
    d[rng.uniform(size=n) < 0.02] = 0.0              # empty places
    return d


def test_query_matches_f64(capi, synth):
    sc = synth.make_scene(200_000, 30_000)
    rng = np.random.default_rng(5)
    with capi.Context() as ctx:
        ctx.map_build(sc["map_xyz"])
        ctx.scan_set(sc["scan_xyz"])
        x = sc["x_true"]
        q = ctx.place_describe(x)
        grid = np.array([[gx, gy, 1.5] for gx in np.arange(-30.0, 31.0, 6.0) for gy in np.arange(-30.0, 31.0, 6.0)])
        ctx.place_add_map(grid)                      # real places first, then random ones and rolled copies of the query
        places = _random_places(rng, 3000)
        rolled = np.stack([np.roll(q, s, axis=1) * np.float32(1.0 + 0.01 * s) for s in range(0, 60, 7)])
        ctx.place_load(places, rng.normal(0, 10, (len(places), 3)))
        ctx.place_load(rolled, np.zeros((len(rolled), 3)))
        desc, _ = ctx.place_fetch()
        n = len(desc)
        ids, shifts, dist = ctx.place_query(x, 64)
    dref, sref, dall = pr.distances(q, desc)
    assert len(ids) == 64
    assert np.all(np.abs(dist.astype(np.float64) - dref[ids]) < 1e-5)
    for i, s in zip(ids, shifts):
        if s != sref[i]:
            second = np.sort(dall[i])[1]
            assert second - dref[i] < 1e-5, (i, s, sref[i])
    kth = np.sort(dref)[63]
    want = set(np.nonzero(dref < kth - 1e-5)[0])
    assert want <= set(ids.tolist())
    assert all(dref[i] <= kth + 1e-5 for i in ids)
    keys = [(float(d), int(i)) for d, i in zip(dist, ids)]
    assert keys == sorted(keys), "ordered by (distance, id)"
    assert n == len(grid) + 3000 + len(rolled)


def test_shift_semantics(capi, synth):
    rects = synth.scene_surfaces(1_000_000)
    scan = synth.ring_sweep(rects, np.eye(3), np.array([10.0, 5.0, 1.5]), 64, 1024)
    x = synth.make_state((0.0, 0.0, 0.0), (0.0, 0.0, 0.0, 1.0))
    rng = np.random.default_rng(9)
    with capi.Context() as ctx:
        ctx.scan_set(scan)
        D = ctx.place_describe(x)
        ctx.place_load(_random_places(rng, 200), np.zeros((200, 3)))
        base = ctx.place_count()
        for s in (7, 30, 53):
            ctx.place_load(np.roll(D, s, axis=1)[None], np.zeros((1, 3)))
        ids, shifts, dist = ctx.place_query(x, 3)
    assert ids.tolist() == [base, base + 1, base + 2]
    assert shifts.tolist() == [7, 30, 53]
    assert np.all(dist <= 1e-6) and len(set(_bits(dist).tolist())) == 1


def test_states_and_limits(capi, synth):
    sc = synth.make_scene(50_000, 2_000)
    x = sc["x_true"]
    xp = x.ctypes.data_as(capi.C.c_void_p)
    C = capi.C
    with capi.Context() as ctx:
        out = np.zeros(20 * 60, np.float32)
        ids = np.zeros(64, np.uint32)
        sh = np.zeros(64, np.int32)
        dd = np.zeros(64, np.float32)
        n = C.c_size_t(0)
        uid = C.c_uint32(0)
        fp = C.POINTER(C.c_float)

        def query(k):
            return _rc(ctx, "lv_place_query", xp, int(k), ids.ctypes.data_as(C.POINTER(C.c_uint32)), sh.ctypes.data_as(C.POINTER(C.c_int32)),
                       dd.ctypes.data_as(fp), C.byref(n))

        # no scan yet
        assert _rc(ctx, "lv_place_describe", xp, out.ctypes.data_as(fp)) == LV_ESTATE
        assert _rc(ctx, "lv_place_add_scan", xp, C.byref(uid)) == LV_ESTATE
        ctx.place_load(np.ones((1, 20, 60), np.float32), np.zeros((1, 3)))
        assert query(4) == LV_ESTATE
        ctx.place_clear()
        ctx.scan_set(sc["scan_xyz"])
        assert query(4) == LV_ESTATE, "empty database"
        for bad in (dict(n_rings=0), dict(n_rings=33), dict(n_sectors=1), dict(n_sectors=65), dict(rmin=-0.5), dict(rmin=80.0),
                    dict(rmin=90.0), dict(rmax=1000.5), dict(rmax=math.inf), dict(rmin=math.nan), dict(z_offset=math.nan),
                    dict(z_offset=-math.inf)):
            p = capi.default_place_params(**bad)
            assert _rc(ctx, "lv_place_configure", C.byref(p)) == LV_EINVAL, bad
        ctx.place_configure(capi.default_place_params(n_rings=32, n_sectors=64, rmin=0.0, rmax=1000.0))
        ctx.place_configure()
        # k limits and clamping
        for _ in range(3):
            ctx.place_add_scan(x)
        assert query(0) == LV_EINVAL and query(65) == LV_EINVAL
        assert query(10) == 0 and n.value == 3 and sorted(ids[:3].tolist()) == [0, 1, 2]
        assert np.all(dd[:3] == dd[0]) and ids[:3].tolist() == [0, 1, 2], "equal places: by id"
        # bad loads change nothing
        for v in (-1.0, math.nan, math.inf):
            bad = np.ones((2, 20, 60), np.float32)
            bad[1, 3, 4] = v
            assert _rc(ctx, "lv_place_load", bad.ctypes.data_as(fp), np.zeros(6).ctypes.data_as(C.POINTER(C.c_double)), 2) == LV_EINVAL
        cen = np.zeros(6)
        cen[4] = math.nan
        assert _rc(ctx, "lv_place_load", np.ones(2400, np.float32).ctypes.data_as(fp), cen.ctypes.data_as(C.POINTER(C.c_double)), 2) == LV_EINVAL
        assert _rc(ctx, "lv_place_add_map", cen.ctypes.data_as(C.POINTER(C.c_double)), 0, None) == LV_EINVAL
        assert _rc(ctx, "lv_place_add_map", np.zeros(3 * 65537).ctypes.data_as(C.POINTER(C.c_double)), 65537, None) == LV_EINVAL
        assert ctx.place_count() == 3
        small = np.zeros(3 * 20 * 60, np.float32)
        assert _rc(ctx, "lv_place_fetch", small.ctypes.data_as(fp), None, 2) == LV_EINVAL
        # fetch -> clear -> load: the same query bit for bit; two identical queries agree
        rng = np.random.default_rng(2)
        ctx.place_load(_random_places(rng, 500), rng.normal(0, 5, (500, 3)))
        ctx.map_build(sc["map_xyz"])
        ctx.place_add_map(np.array([[0.0, 0.0, 1.5], [10.0, -4.0, 1.0], [-20.0, 7.0, 2.0]]))
        a = ctx.place_query(x, 64)
        b = ctx.place_query(x, 64)
        desc, cen = ctx.place_fetch()
        ctx.place_clear()
        assert ctx.place_count() == 0
        ctx.place_load(desc, cen)
        c = ctx.place_query(x, 64)
        for u, v in ((a, b), (a, c)):
            assert np.array_equal(u[0], v[0]) and np.array_equal(u[1], v[1]) and np.array_equal(_bits(u[2]), _bits(v[2]))
        d2, c2 = ctx.place_fetch()
        assert np.array_equal(_bits(d2), _bits(desc)) and np.array_equal(c2, cen)
        # 2^20 places at most
        ctx.place_configure(capi.default_place_params(n_rings=1, n_sectors=2))
        ctx.place_load(np.ones((1 << 20, 1, 2), np.float32), np.zeros(((1 << 20), 3)))
        assert _rc(ctx, "lv_place_load", np.ones(2, np.float32).ctypes.data_as(fp), np.zeros(3).ctypes.data_as(C.POINTER(C.c_double)), 1) == LV_ERANGE
        assert _rc(ctx, "lv_place_add_scan", xp, None) == LV_ERANGE
        assert _rc(ctx, "lv_place_add_map", np.zeros(3).ctypes.data_as(C.POINTER(C.c_double)), 1, None) == LV_ERANGE
        assert ctx.place_count() == 1 << 20
        ids, _, _ = ctx.place_query(x, 5)
        assert ids.tolist() == [0, 1, 2, 3, 4]


def test_add_map_is_read_only(capi, synth):
    sc = synth.make_scene(200_000, 1_000)
    centres = np.array([[gx, gy, 1.5] for gx in np.arange(-20.0, 21.0, 10.0) for gy in np.arange(-20.0, 21.0, 10.0)])
    with capi.Context() as ctx:
        ctx.map_build(sc["map_xyz"])
        ctx.map_evict_box(np.array([-5.0, -5.0, -1.0], np.float32), np.array([5.0, 5.0, 10.0], np.float32), keep_inside=False)
        before = ctx.map_fetch()
        ctx.place_add_map(centres)
        assert np.array_equal(_bits(ctx.map_fetch()), _bits(before))
        ref, _ = ctx.place_fetch()
        ctx.map_relinearise_async()
        ctx.place_add_map(centres)
        during = ctx.map_fetch()
        ctx.map_rebuild_status(wait=True)
        assert np.array_equal(_bits(during), _bits(before)) and np.array_equal(_bits(ctx.map_fetch()), _bits(before))
        desc, _ = ctx.place_fetch()
    assert np.array_equal(_bits(desc[len(centres):]), _bits(ref)), "the same places beside a background rebuild"
    for i in (0, 12, 24):
        want, und = pr.describe(pr.map_q(before, centres[i]), tol_rad=TOL_RAD)
        _compare(ref[i], want, und, f"evicted map, centre {i}")


# ---- end to end: a 1 M-point scene, no pose prior

def _boxes(rects):
    o, eu, ev = rects
    return [(o[i][0], o[i][1], o[i][0] + eu[i][0], o[i][1] + ev[i][1]) for i in range(5, len(o), 5)]


def _free(p, boxes, margin=1.5):
    return all(not (x0 - margin <= p[0] <= x1 + margin and y0 - margin <= p[1] <= y1 + margin) for x0, y0, x1, y1 in boxes)


@pytest.fixture(scope="module")
def world(synth):
    sc = synth.make_scene(1_000_000, 1_000)
    rects = synth.scene_surfaces(1_000_000)
    boxes = _boxes(rects)
    L = sc["L"]
    path = [np.array([x, -10.0, 1.5]) for x in np.arange(-50.0, 51.0, 5.0)]
    keyframes = [p for p in path if _free(p, boxes)]
    rng = np.random.default_rng(17)
    yaws = np.radians([-172.0, -110.0, -41.0, 23.0, 96.0, 158.0])
    queries = []
    while len(queries) < 6:
        k = keyframes[int(rng.integers(len(keyframes)))]
        a, r = rng.uniform(-math.pi, math.pi), rng.uniform(0.5, 2.0)
        p = k + np.array([r * math.cos(a), r * math.sin(a), 0.0])
        d = min(np.linalg.norm(p[:2] - kk[:2]) for kk in keyframes)
        if _free(p, boxes) and 0.5 <= d <= 2.0:
            queries.append((p, float(yaws[len(queries)])))
    w = dict(sc=sc, rects=rects, L=L, keyframes=keyframes, queries=queries)
    w["kf_scans"] = [_sweep(synth, w, k, 0.0) for k in keyframes]
    w["q_scans"] = [_sweep(synth, w, p, yaw) for p, yaw in queries]
    return w


def _sweep(synth, w, p, yaw):
    return synth.ring_sweep(w["rects"], synth.quat_to_rot(synth.quat_from_rpy(0.0, 0.0, yaw)), p, 64, 1024)


def _err(synth, est, p, yaw):
    qt = synth.quat_from_rpy(0.0, 0.0, yaw)
    ang = math.degrees(2 * math.acos(min(1.0, abs(float(np.dot(est[3:7], qt))))))
    return float(np.linalg.norm(est[:3] - p)), ang


def test_relocalise_from_keyframes(capi, synth, world):
    from limo_velo_amd import places

    w = world
    x_level = synth.make_state((0.0, 0.0, 0.0), (0.0, 0.0, 0.0, 1.0))
    P0 = synth.default_P0()
    top1, errs = 0, []
    with capi.Context() as ctx:
        ctx.map_build(w["sc"]["map_xyz"])
        for k, scan in zip(w["keyframes"], w["kf_scans"]):
            ctx.scan_set(scan)
            ctx.place_add_scan(synth.make_state(k, (0.0, 0.0, 0.0, 1.0)))
        assert ctx.place_count() == len(w["keyframes"])
        for (p, yaw), scan in zip(w["queries"], w["q_scans"]):
            ctx.scan_downsample(scan, 0.5)
            ids, shifts, _ = ctx.place_query(x_level, 8)
            near = int(np.argmin([np.linalg.norm(p[:2] - k[:2]) for k in w["keyframes"]]))
            dyaw = abs(math.remainder(pr.shift_yaw(int(shifts[0]), 60) - yaw, 2 * math.pi))
            top1 += int(ids[0] == near and dyaw <= 2 * math.pi / 60)
            best, table = places.global_localise(ctx, x_level, P0, k=8)
            errs.append(_err(synth, best, p, yaw))
    print("keyframes: top-1", top1, "of 6; errors (m, deg)", errs)
    assert top1 >= 5, (top1, errs)
    assert all(e[0] < 0.02 and e[1] < 0.2 for e in errs), errs


def test_relocalise_from_map_places(capi, synth, world):
    from limo_velo_amd import places

    w = world
    x_level = synth.make_state((0.0, 0.0, 0.0), (0.0, 0.0, 0.0, 1.0))
    P0 = synth.default_P0()
    centres = places.map_grid_centres(w["sc"]["map_xyz"], 4.0, 1.5)
    hits, errs = 0, []
    with capi.Context() as ctx:
        ctx.map_build(w["sc"]["map_xyz"])
        ctx.place_add_map(centres)
        for (p, yaw), scan in zip(w["queries"], w["q_scans"]):
            ctx.scan_downsample(scan, 0.5)
            ids, _, _ = ctx.place_query(x_level, 16)
            near = int(np.argmin(np.linalg.norm(centres[:, :2] - p[:2], axis=1)))
            if near in ids.tolist():
                hits += 1
                best, _ = places.global_localise(ctx, x_level, P0, k=16, xy_radius=3.0, xy_step=1.0)
                errs.append(_err(synth, best, p, yaw))
    print("map places:", len(centres), "centres; nearest in the top 16 for", hits, "of 6; errors (m, deg)", errs)
    assert hits >= 4, (hits, errs)
    assert all(e[0] < 0.02 and e[1] < 0.2 for e in errs), errs
