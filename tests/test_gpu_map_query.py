"""GPU tests of the map queries (lv_map_knn / lv_map_radius_search / lv_map_box_search, lv_query.hip) against brute force.

Brute force is the CPU oracle's lvo_knn_brute (k <= 15: its TopK keeps k + 1 <= 16 entries) or, for larger k and for the
radius / box queries, a numpy restatement of the reference's calc_dist (f32, (dx^2 + dy^2) + dz^2, unfused) with a sort on
(d2, index); the restatement is itself held to lvo_knn_brute.  Indices are ranks among the living points (map_fetch order)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NONE = np.uint32(0xFFFFFFFF)


@pytest.fixture(scope="module")
def capi(lv):
    from limo_velo_amd import capi as c

    return c


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def calc_dist(q, m):
    """[nq, 3] x [nm, 3] -> [nq, nm] f32 squared distances in calc_dist's operation order."""
    q = np.asarray(q, np.float32)[:, None, :]
    m = np.asarray(m, np.float32)[None, :, :]
    d = q - m
    with np.errstate(invalid="ignore", over="ignore"):
        s = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]
        return s + d[..., 2] * d[..., 2]


def np_knn(map_xyz, q, k, max_dist=np.inf, chunk=64):
    """(idx, d2, found) by brute force on (d2, index); admitted iff d2 finite and d2 <= f32(max_dist)^2 (f32)."""
    map_xyz = np.asarray(map_xyz, np.float32)
    q = np.asarray(q, np.float32)
    md = np.float32(max_dist)
    with np.errstate(over="ignore"):
        max_d2 = md * md
    n, m = len(q), len(map_xyz)
    idx = np.full((n, k), NONE, np.uint32)
    d2 = np.full((n, k), np.inf, np.float32)
    ar = np.arange(m, dtype=np.uint64)
    for s in range(0, n, chunk):
        d = calc_dist(q[s:s + chunk], map_xyz)
        ok = np.isfinite(d) & (d <= max_d2)
        key = np.where(ok, (d.view(np.uint32).astype(np.uint64) << np.uint64(32)) | ar, np.uint64(~np.uint64(0)))
        kk = min(k, m)
        if m > kk:
            key = np.partition(key, kk - 1, axis=1)[:, :kk]
        key = np.sort(key, axis=1)[:, :kk]
        real = key != np.uint64(~np.uint64(0))
        idx[s:s + chunk, :kk] = np.where(real, (key & np.uint64(0xFFFFFFFF)).astype(np.uint32), NONE)
        d2[s:s + chunk, :kk] = np.where(real, (key >> np.uint64(32)).astype(np.uint32).view(np.float32), np.float32(np.inf))
    return idx, d2, (idx != NONE).sum(axis=1).astype(np.int32)


def _assert_knn_equal(got, want):
    gi, gd, gf = got
    wi, wd, wf = want
    bad = (gi != wi).any(axis=1) | (_bits(gd) != _bits(wd)).any(axis=1)
    assert not bad.any(), f"{bad.sum()} of {len(bad)} queries differ; first {np.flatnonzero(bad)[:5]}: {gi[bad][:2]} vs {wi[bad][:2]}"
    assert np.array_equal(gf, wf)


def _queries(map_xyz, n, seed=1):
    """Map points jittered by a few cm to a few m, points on a 0.25 m lattice (voxel walls), far-off points (inside and beyond
    the voxel range: CELL_FAR = 2^19 voxels of 0.5 m) and non-finite ones."""
    rng = np.random.default_rng(seed)
    base = map_xyz[rng.integers(0, len(map_xyz), n)]
    jit = base + rng.normal(0, 1, (n, 3)).astype(np.float32) * rng.choice([0.02, 0.3, 2.0], (n, 1)).astype(np.float32)
    wall = (np.round(base[: n // 4] * 4) / 4 + np.float32(1e-5)).astype(np.float32)
    far = np.array([[80, 0, 0], [0, -150, 3], [3.0e5, 0, 0], [-1.0e6, 2.0e5, 10]], np.float32)
    bad = np.array([[np.nan, 0, 0], [np.inf, 1, 1], [0, -np.inf, 0]], np.float32)
    return np.concatenate([jit, wall, far, bad]).astype(np.float32)


@pytest.fixture(scope="module")
def cfg0(capi, scene_small):
    m = np.asarray(scene_small["map_xyz"], np.float32)
    q = _queries(m, 1500)
    ctx = capi.Context()
    ctx.map_build(m)
    yield ctx, m, q
    ctx.close()


@pytest.mark.parametrize("k", [1, 5, 8, 16, 32])
def test_knn_parity_cfg0(cfg0, oracle, k):
    ctx, m, q = cfg0
    got = ctx.map_knn(q, k)
    if k <= 15:
        bi, bd, bf, _ = oracle.knn_brute(m, q, k)
        _assert_knn_equal(got, (bi, bd, bf))
    else:
        _assert_knn_equal(got, np_knn(m, q, k))
        bi, bd, bf, _ = oracle.knn_brute(m, q, 15)   # the restatement against the oracle on the same queries
        _assert_knn_equal(np_knn(m, q, 15), (bi, bd, bf))
    assert (got[2][-3:] == 0).all(), "non-finite queries find nothing"
    assert (got[2][:-3] == min(k, len(m))).all()


def test_knn_matches_the_update_search(capi, cfg0, synth_state_identity):
    """NUM_MATCH_POINTS = 5, identity state: lv_map_knn(q, 5) == lv_scan_set(q) + lv_iterate + lv_fetch_knn, bit for bit."""
    _, m, q = cfg0
    q = q[:-3]   # (finite queries: the update's own search reports a non-finite point differently)
    with capi.Context() as ctx:
        ctx.map_build(m)
        ctx.scan_set(q)
        ctx.iterate(synth_state_identity)
        ui, ud = ctx.fetch_knn()
        gi, gd, _ = ctx.map_knn(q, 5)
    assert np.array_equal(gi, ui)
    assert np.array_equal(_bits(gd), _bits(ud))


@pytest.fixture(scope="module")
def synth_state_identity():
    from limo_velo_amd import synth

    return synth.make_state((0, 0, 0), (0, 0, 0, 1))


@pytest.mark.parametrize("scale", [3.0, 8.0])
def test_knn_with_the_pose_off(capi, oracle, scale):
    """Queries from a scan placed with the pose 3x / 8x off (as test_gpu_parity's pruning test): many leave the bucket levels."""
    from limo_velo_amd import synth

    sc = synth.make_scene(300_000, 6_000)
    x0 = np.array(sc["x_true"], np.float64).copy()
    x0[:3] += scale * (np.array(sc["x_init"][:3]) - np.array(sc["x_true"][:3]))
    qt, qi = np.array(sc["x_true"][3:7]), np.array(sc["x_init"][3:7])
    qq = qt + scale * (qi - qt)
    x0[3:7] = qq / np.linalg.norm(qq)
    q = oracle.transform_scan(x0, sc["scan_xyz"])
    tree = oracle.KdTree(sc["map_xyz"])
    with capi.Context() as ctx:
        ctx.map_build(sc["map_xyz"])
        for k in (5, 8):
            _assert_knn_equal(ctx.map_knn(q, k), tree.knn(q, k))


def test_knn_lattice_ties_by_index(capi, oracle):
    g = np.arange(12, dtype=np.float32)
    m = np.stack(np.meshgrid(g, g, np.arange(4, dtype=np.float32), indexing="ij"), -1).reshape(-1, 3)
    q = np.concatenate([m[::7], m[::5] + np.float32(0.5), m[::3] + np.array([0.5, 0, 0], np.float32)]).astype(np.float32)
    with capi.Context() as ctx:
        ctx.map_build(m)
        for k in (5, 8):
            bi, bd, bf, ties = oracle.knn_brute(m, q, k)
            assert ties > 0
            _assert_knn_equal(ctx.map_knn(q, k), (bi, bd, bf))
        _assert_knn_equal(ctx.map_knn(q, 27), np_knn(m, q, 27))


def test_knn_small_and_empty_maps(capi):
    q = np.array([[0, 0, 0], [1, 2, 3], [50, 50, 50]], np.float32)
    with capi.Context() as ctx:
        idx, d2, found = ctx.map_knn(q, 32)   # no map yet
        assert (idx == NONE).all() and np.isinf(d2).all() and (found == 0).all()
        off, total = ctx.map_radius_count(q, 5.0)
        assert total == 0 and (off == 0).all()
        assert len(ctx.map_box([-1e9] * 3, [1e9] * 3)[0]) == 0
        m = np.random.default_rng(3).uniform(-2, 2, (10, 3)).astype(np.float32)
        ctx.map_build(m)
        got = ctx.map_knn(q, 32)
        assert (got[2] == 10).all()
        _assert_knn_equal(got, np_knn(m, q, 32))


def test_knn_argument_checks(capi, cfg0):
    ctx, _, q = cfg0
    for k in (0, 33, -1):
        with pytest.raises(capi.LvError):
            ctx.map_knn(q[:4], k)
    for md in (-1.0, np.nan):
        with pytest.raises(capi.LvError):
            ctx.map_knn(q[:4], 5, max_dist=md)
    with pytest.raises(capi.LvError):
        ctx.map_radius(q[:4], -1.0)


def test_knn_max_dist(cfg0, oracle):
    ctx, m, q = cfg0
    for md in (0.05, 0.3, 1.5):
        _assert_knn_equal(ctx.map_knn(q, 8, max_dist=md), np_knn(m, q, 8, max_dist=md))
    # the inclusive boundary: a max_dist whose f32 square is exactly some neighbour's d2
    bi, bd, _, _ = oracle.knn_brute(m, q[:-3], 8)
    cand = np.sqrt(bd[:, 3].astype(np.float64)).astype(np.float32)
    exact = np.flatnonzero((cand * cand == bd[:, 3]) & (bd[:, 3] > 0))
    assert len(exact) > 0
    j = exact[0]
    md = float(cand[j])
    got = ctx.map_knn(q[j:j + 1], 8, max_dist=md)
    assert got[0][0, 3] == bi[j, 3] and _bits(got[1])[0, 3] == _bits(bd)[j, 3]
    _assert_knn_equal(ctx.map_knn(q, 8, max_dist=md), np_knn(m, q, 8, max_dist=md))


def test_knn_after_incremental_inserts(capi, oracle, scene_small):
    """Inserts that break tile groups up (extent 0: the level-1 region is skipped) and the searches that follow."""
    m = np.asarray(scene_small["map_xyz"], np.float32)
    rng = np.random.default_rng(5)
    with capi.Context() as ctx:
        ctx.map_build(m[:20_000])
        for s in range(20_000, len(m), 6_000):
            ctx.map_add(m[s:s + 6_000] + rng.normal(0, 0.05, (len(m[s:s + 6_000]), 3)).astype(np.float32))
        live = ctx.map_fetch()
        q = _queries(live, 1000, seed=6)
        for k in (5, 16):
            _assert_knn_equal(ctx.map_knn(q, k), np_knn(live, q, k))


def test_knn_after_evictions(capi, scene_small):
    m = np.asarray(scene_small["map_xyz"], np.float32)
    with capi.Context() as ctx:
        ctx.map_build(m)
        c = np.median(m, axis=0)
        assert ctx.map_evict_box(c - 6, c + 6, keep_inside=False) > 0
        assert ctx.map_evict_oldest(5_000) == 5_000
        live = ctx.map_fetch()
        q = _queries(live, 1000, seed=7)
        q = np.concatenate([q, np.repeat(c[None], 8, 0).astype(np.float32)])   # inside the hole
        for k in (5, 32):
            got = ctx.map_knn(q, k)
            _assert_knn_equal(got, np_knn(live, q, k))
            idx, d2, _ = got
            ok = idx != NONE
            qq = np.repeat(q[:, None, :], k, 1)[ok]
            d = qq - live[idx[ok]]
            rec = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
            assert np.array_equal(_bits(rec), _bits(d2[ok])), "map_fetch()[idx] does not reproduce d2"


def _np_radius(m, q, r):
    rr = np.float32(r) * np.float32(r)
    off, idx, d2 = [0], [], []
    for s in range(0, len(q), 64):
        d = calc_dist(q[s:s + 64], m)
        for row in d:
            hit = np.flatnonzero(np.isfinite(row) & (row <= rr))
            idx.append(hit.astype(np.uint32))
            d2.append(row[hit])
            off.append(off[-1] + len(hit))
    return np.array(off, np.uint64), np.concatenate(idx), np.concatenate(d2).astype(np.float32)


@pytest.mark.parametrize("r", [0.3, 1.0, 2.5, 10.0])
def test_radius_search(cfg0, capi, r):
    ctx, m, q = cfg0
    q = q[:: (1 if r < 5 else 8)]
    off, idx, d2 = ctx.map_radius(q, r)
    wo, wi, wd = _np_radius(m, q, r)
    assert np.array_equal(off, wo)
    assert np.array_equal(idx, wi)
    assert np.array_equal(_bits(d2), _bits(wd))
    o2, total = ctx.map_radius_count(q, r)
    assert total == int(wo[-1]) and np.array_equal(o2, wo)
    if total > 1:   # too small a capacity: LV_EINVAL, offsets / total still written
        a = np.ascontiguousarray(q, np.float32)
        offs = np.zeros(len(q) + 1, np.uint64)
        t = C.c_size_t(0)
        buf = np.empty(total - 1, np.uint32)
        rc = ctx.lib.lv_map_radius_search(ctx.h, a.ctypes.data_as(C.c_void_p), C.c_size_t(12), C.c_size_t(len(q)), C.c_float(r),
                                          offs.ctypes.data_as(C.POINTER(C.c_size_t)), buf.ctypes.data_as(C.POINTER(C.c_uint32)), None,
                                          C.c_size_t(total - 1), C.byref(t))
        assert rc == -1 and t.value == total and np.array_equal(offs, wo)


def test_box_search_equals_the_eviction(capi, scene_small):
    m = np.asarray(scene_small["map_xyz"], np.float32)
    c = np.median(m, axis=0)
    lo, hi = (c - np.array([8, 5, 1])).astype(np.float32), (c + np.array([3, 9, 2])).astype(np.float32)
    lo[0] = m[100, 0]   # a point on the lower face: inclusive
    with capi.Context() as a, capi.Context() as b:
        a.map_build(m)
        b.map_build(m)
        a.map_evict_oldest(1_000)
        b.map_evict_oldest(1_000)
        live = a.map_fetch()
        idx, xyz = a.map_box(lo, hi)
        want = np.flatnonzero(((live >= lo) & (live <= hi)).all(axis=1))
        assert len(want) > 0 and np.array_equal(idx, want.astype(np.uint32))
        assert np.array_equal(xyz, live[want])
        n = b.map_evict_box(lo, hi, keep_inside=False)
        assert n == len(idx)
        assert np.array_equal(b.map_fetch(), np.delete(live, idx, axis=0))
        cnt = C.c_size_t(0)
        small = np.empty(max(len(idx) - 1, 1), np.uint32)
        fp = C.POINTER(C.c_float)
        rc = a.lib.lv_map_box_search(a.h, lo.ctypes.data_as(fp), hi.ctypes.data_as(fp), small.ctypes.data_as(C.POINTER(C.c_uint32)), None,
                                     C.c_size_t(len(idx) - 1), C.byref(cnt))
        assert rc == -1 and cnt.value == len(idx)


def test_query_right_after_an_insert_sees_it(capi, oracle, scene_small, synth_state_identity):
    """lv_map_add_scan returns before the insert (side stream) has run; the query that follows must see it."""
    from limo_velo_amd import synth

    m = np.asarray(scene_small["map_xyz"], np.float32)
    scan = np.asarray(scene_small["scan_xyz"], np.float32) + np.float32(0.013)
    with capi.Context() as ctx:
        ctx.map_build(m)
        ctx.filter_set(synth_state_identity, synth.default_P0())
        ctx.scan_set(scan)
        ctx.map_add_scan(downsample=False)
        got = ctx.map_knn(scan, 5)
        live = ctx.map_fetch()
    assert len(live) == len(m) + len(scan)
    _assert_knn_equal(got, np_knn(live, scan, 5))
    assert (got[1][:, 0] == 0).all()


def test_queries_beside_a_background_rebuild(capi, oracle):
    from limo_velo_amd import synth

    sc = synth.make_scene(300_000, 2_000)
    m = np.asarray(sc["map_xyz"], np.float32)
    q = oracle.transform_scan(sc["x_init"], sc["scan_xyz"])
    with capi.Context() as ctx:
        ctx.map_build(m)
        assert ctx.map_evict_oldest(100_000) == 100_000
        live = ctx.map_fetch()
        tree = oracle.KdTree(live)
        want = tree.knn(q, 5)
        ctx.map_relinearise_async()
        _assert_knn_equal(ctx.map_knn(q, 5), want)   # the active store, rebuild in flight
        st = ctx.map_rebuild_status(wait=True)
        assert st["started"] >= 1
        _assert_knn_equal(ctx.map_knn(q, 5), want)   # adopted: ids compacted, ranks unchanged
        assert ctx.map_rebuild_status()["adopted"] >= 1
        _assert_knn_equal(ctx.map_knn(q[:256], 16), np_knn(live, q[:256], 16))


def test_headline_scale(capi, oracle):
    """The bench scene: 1 M-point map, 65 536 queries placed like the headline scan."""
    from limo_velo_amd import synth

    sc = synth.make_scene(1_000_000, 65_536)
    m = np.asarray(sc["map_xyz"], np.float32)
    q = oracle.transform_scan(sc["x_init"], sc["scan_xyz"])
    with capi.Context() as ctx:
        ctx.map_build(m)
        got = ctx.map_knn(q, 5)
        sub = ctx.map_knn(q[:4096], 32)
    # k = 5: every query against the oracle's exact kd-tree (an independent CPU search), the first 512 also against lvo_knn_brute
    # (1 M x 65 536 brute-force distances would take minutes)
    _assert_knn_equal(got, oracle.KdTree(m).knn(q, 5))
    bi, bd, bf, _ = oracle.knn_brute(m, q[:512], 5)
    _assert_knn_equal(tuple(a[:512] for a in got), (bi, bd, bf))
    # k = 32 on a 4096-query subset: the numpy restatement over every map point that can be among the 32 nearest (slab search,
    # exhaustive: see _np_knn_slab), and over the whole map for the first 256
    _assert_knn_equal(sub, _np_knn_slab(m, q[:4096], 32, sub))
    _assert_knn_equal(tuple(a[:256] for a in sub), np_knn(m, q[:256], 32, chunk=16))


def _np_knn_slab(m, q, k, got):
    """The numpy restatement of k-NN restricted to the map points whose x lies within R of the query's, R = the distance of the
    k-th neighbour the device reported.  Those k neighbours are map points at the distances reported (checked first), so the true
    k-th distance is <= R and every point of the true answer lies inside the slab: the restatement over the slab is exhaustive.
    Queries with fewer than k neighbours fall back to the whole map."""
    gi, gd, gf = got
    order = np.argsort(m[:, 0], kind="stable")
    xs = m[order, 0]
    idx = np.full((len(q), k), NONE, np.uint32)
    d2 = np.full((len(q), k), np.inf, np.float32)
    for i in range(len(q)):
        if gf[i] < k:
            wi, wd, _ = np_knn(m, q[i:i + 1], k)
            idx[i], d2[i] = wi[0], wd[0]
            continue
        rec = calc_dist(q[i:i + 1], m[gi[i]])[0]
        assert np.array_equal(_bits(rec), _bits(gd[i])), f"query {i}: reported distances are not those of the reported points"
        r = float(np.sqrt(np.float64(gd[i, k - 1]))) * 1.001 + 1e-4
        cand = order[np.searchsorted(xs, q[i, 0] - r, "left"):np.searchsorted(xs, q[i, 0] + r, "right")]
        d = calc_dist(q[i:i + 1], m[cand])[0]
        key = np.sort((d.view(np.uint32).astype(np.uint64) << np.uint64(32)) | cand.astype(np.uint64))[:k]
        idx[i] = (key & np.uint64(0xFFFFFFFF)).astype(np.uint32)
        d2[i] = (key >> np.uint64(32)).astype(np.uint32).view(np.float32)
    return idx, d2, (idx != NONE).sum(axis=1).astype(np.int32)


def test_radius_totals_beyond_32_bits(capi, scene_small):
    """A radius search whose total passes 2^32 (90 000 queries that each find all 50 000 points: 4.5e9): the count-only call
    reports the exact 64-bit offsets and total, and the fill — whose device sort counts in an int — is refused with LV_EINVAL
    before anything is allocated or written (the buffer handed in is never touched: the call checks first)."""
    m = np.asarray(scene_small["map_xyz"], np.float32)
    n = 90_000
    q = np.repeat(np.median(m, axis=0, keepdims=True), n, 0).astype(np.float32)
    with capi.Context() as ctx:
        ctx.map_build(m)
        off, total = ctx.map_radius_count(q, 1.0e6)
        assert total == n * len(m) > 2**32
        assert np.array_equal(off, np.arange(n + 1, dtype=np.uint64) * np.uint64(len(m)))
        offs = np.zeros(n + 1, np.uint64)
        t = C.c_size_t(0)
        one = np.empty(1, np.uint32)
        rc = ctx.lib.lv_map_radius_search(ctx.h, q.ctypes.data_as(C.c_void_p), C.c_size_t(12), C.c_size_t(n), C.c_float(1.0e6),
                                          offs.ctypes.data_as(C.POINTER(C.c_size_t)), one.ctypes.data_as(C.POINTER(C.c_uint32)), None,
                                          C.c_size_t(total), C.byref(t))
        assert rc == -1 and t.value == total and np.array_equal(offs, off)
        assert b"at most" in ctx.lib.lv_last_error()
        # the context is still good: an ordinary search right after
        o2, i2, _ = ctx.map_radius(q[:3], 0.5)
        assert o2[-1] == len(i2)
