"""The id-ordered level-1 neighbourhood buckets (DESIGN section 3 "Level 1"): the 5-NN search probes bt[1] and streams the
bucket of the query's level-1 voxel; position order there is the reference's index order, ties included.  Every test holds
idx and d2 to the CPU oracle bit for bit, on the capturing path (lv_iterate / lv_fetch_knn) and on the timed one (lv_update
with the records dumped / lv_fetch_neighbors), with the pose pushed far enough off that level 0 cannot decide a large share
of the scan — a share that is computed here, on the CPU, from the oracle's d5 and the documented radius rule
(level l accepts iff d5 < r_l^2, lv_search_dev.hpp search_radius) before anything runs on the GPU."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CELL = np.float32(0.5)          # lv_default_params: voxel_size
CELL_OFFSET = 1 << 20


@pytest.fixture(scope="module")
def capi(lv):
    from limo_velo_amd import capi as c

    return c


@pytest.fixture(scope="module")
def scene(lv):
    from limo_velo_amd import synth

    return synth.make_scene(20_000, 1024)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _origin(map_xyz):
    """MapStore::rebuild: the bounding box's centre snapped to the level-0 lattice (f32)."""
    lo, hi = map_xyz.min(0).astype(np.float32), map_xyz.max(0).astype(np.float32)
    return (np.floor(np.float32(0.5) * (lo + hi) / CELL) * CELL).astype(np.float32)


def _radius_sq(q, origin, lvl):
    """search_radius (lv_search_dev.hpp) in f32, squared as the kernel squares it."""
    f = np.float32
    inv = f(1.0) / CELL
    t = ((q - origin) * inv).astype(np.float32)
    c0 = np.floor(t).astype(np.int64) + CELL_OFFSET
    amax = np.abs(c0 - CELL_OFFSET).max(axis=1).astype(np.float32)
    scale = f(1 << lvl)
    b = (((c0 >> lvl) << lvl) - CELL_OFFSET).astype(np.float32)
    m = np.minimum(t - b, scale - (t - b)).min(axis=1)
    marg = np.maximum(m, f(0)).astype(np.float32)
    r = CELL * ((scale + marg) * f(0.999) - f(8.0) * f(1.1920928955078125e-07) * (amax + f(2.0) * scale))
    r = r.astype(np.float32)
    return (r * r).astype(np.float32)


def _fails(oracle, ref, origin, state, scan):
    """per scan point: the oracle's answer and whether levels 0 / 1 cannot accept it"""
    q = oracle.transform_scan(state, scan)
    oi, od, _, _ = oracle.knn_brute(ref, q)
    d5 = od[:, 4]
    return oi, od, ~(d5 < _radius_sq(q, origin, 0)), ~(d5 < _radius_sq(q, origin, 1))


def _off_pose(sc, off):
    x = np.array(sc["x_init"], np.float64).copy()
    x[:3] += off * np.array([1.0, -0.5, 0.3])
    return x


def _check_both_paths(capi, ctx, oracle, ref, origin, state, scan, sc, min_share=0.25, want_l1_fail=True):
    oi, od, f0, f1 = _fails(oracle, ref, origin, state, scan)
    # the oracle alone says level 1 is exercised (checked on the CPU, before the GPU runs)
    assert f0.mean() >= min_share, f0.mean()
    if want_l1_fail:
        assert (f0 & f1).sum() >= 1
    assert (f0 & ~f1).sum() >= 1
    ctx.scan_set(scan)
    ctx.iterate(state)                                   # capturing path
    idx, d2 = ctx.fetch_knn()
    hist = ctx.level_histogram()
    bad = (idx != oi).any(axis=1)
    assert not bad.any(), f"kNN indices differ at {bad.sum()} points"
    assert np.array_equal(_bits(d2), _bits(od))
    assert hist[1] > 0, hist                             # level 1 decided points
    ctx.set_record_dump(True)                            # timed path: the one-launch pass, records also stored
    ctx.update(state, sc["P0"])
    nbr, td2, _, found = ctx.fetch_neighbors()
    ctx.set_record_dump(False)
    max_d2 = float(ctx.params.MAX_DIST_PLANE) ** 2
    near = od[:, 4].astype(np.float64) < max_d2          # (a bounded launch reports no neighbours beyond the plane gate)
    assert (found[near] == 5).all()
    assert np.array_equal(_bits(nbr[near]), _bits(ref[oi[near]])), "timed path: neighbour coordinates differ"
    assert np.array_equal(_bits(td2[near]), _bits(od[near]))
    return f0, f1, hist


def test_level1_is_exercised_and_exact(capi, oracle, scene):
    sc = scene
    ref, origin = sc["map_xyz"], _origin(sc["map_xyz"])
    state = _off_pose(sc, 1.2)
    with capi.Context(capi.default_params(MAX_NUM_ITERS=0)) as ctx:
        ctx.map_build(ref)
        f0, f1, hist = _check_both_paths(capi, ctx, oracle, ref, origin, state, sc["scan_xyz"], sc)
    print(f"\n{f0.sum()} of {len(f0)} points fail level 0, {(f0 & f1).sum()} also level 1; histogram {hist[:6]}")


def test_ties_are_decided_at_level1_in_id_order(capi, oracle):
    """A lattice map (spacing 0.25 m: every coordinate and every squared distance exact in f32): a query near a lattice
    point has bit-equal distances among its six nearest.  Shuffled ids, so that id order is not storage order; the pose sits
    0.95 m above the top layer: d5 is beyond level 0's radius and inside level 1's."""
    rng = np.random.default_rng(4)
    g = np.stack(np.meshgrid(np.arange(-24, 25), np.arange(-24, 25), np.arange(0, 2), indexing="ij"), -1).reshape(-1, 3)
    ref = (g[rng.permutation(len(g))] * 0.25).astype(np.float32)
    origin = _origin(ref)
    # queries exactly above lattice points / edge midpoints / cell centres: 4-fold and 2-fold ties
    base = (g[(np.abs(g[:, 0]) < 16) & (np.abs(g[:, 1]) < 16) & (g[:, 2] == 1)][:900] * 0.25).astype(np.float32)
    shift = np.array([[0, 0, 0], [0.125, 0, 0], [0.125, 0.125, 0]], np.float32)[np.arange(len(base)) % 3]
    scan = (base + shift + np.array([0, 0, 0.9375], np.float32)).astype(np.float32)
    ident = np.zeros(26)
    ident[6] = 1.0
    ident[10] = 1.0
    oi, od, f0, f1 = _fails(oracle, ref, origin, ident, scan)
    q = oracle.transform_scan(ident, scan)
    assert np.array_equal(_bits(q), _bits(scan))         # identity pose: the queries are the scan, exactly
    ties = (od[:, :4] == od[:, 1:5]).any(axis=1)
    assert ties.mean() > 0.9, ties.mean()
    assert (f0 & ~f1).mean() > 0.9, ((f0 & ~f1).mean())  # level 1 decides them
    with capi.Context(capi.default_params(MAX_NUM_ITERS=0)) as ctx:
        ctx.map_build(ref)
        ctx.scan_set(scan)
        ctx.iterate(ident)
        idx, d2 = ctx.fetch_knn()
        hist = ctx.level_histogram()
        assert np.array_equal(idx, oi), f"{(idx != oi).any(axis=1).sum()} points differ from the oracle's (distance, index) order"
        assert np.array_equal(_bits(d2), _bits(od))
        assert hist[1] >= int(0.9 * len(scan)), hist
        ctx.set_record_dump(True)
        ctx.update(ident, np.eye(23) * 1e-4)
        nbr, td2, _, found = ctx.fetch_neighbors()
        assert (found == 5).all()
        assert np.array_equal(_bits(nbr), _bits(ref[oi])) and np.array_equal(_bits(td2), _bits(od))


def _voxel1(p, origin):
    c0 = np.floor(((p - origin) / CELL).astype(np.float32)).astype(np.int64)
    return c0 >> 1


def test_upkeep_of_level1(capi, oracle, scene):
    sc = scene
    ref, origin = sc["map_xyz"], _origin(sc["map_xyz"])
    state, scan = _off_pose(sc, 1.2), sc["scan_xyz"]
    rng = np.random.default_rng(9)
    with capi.Context(capi.default_params(MAX_NUM_ITERS=0)) as ctx:
        ctx.map_build(ref)
        st0 = ctx.map_stats()
        # 1. relocation: the fullest level-1 voxel V takes as many new points as its whole 27-block holds — more than the slack
        # (half the count, at least 8) of the bucket around V — all strictly inside V, so no new level-1 bucket appears and
        # whatever the level-1 pool hands out is room for runs that moved
        v1 = _voxel1(ref, origin)
        keys, inv, cnt = np.unique(v1, axis=0, return_inverse=True, return_counts=True)
        V = keys[np.argmax(cnt)]
        n27 = int((np.abs(v1 - V).max(axis=1) <= 1).sum())
        lo = origin + (V * 2).astype(np.float32) * CELL
        batch = (lo + rng.uniform(0.05, 0.95, (n27, 3)).astype(np.float32)).astype(np.float32)   # V's edge is 1 m
        assert (_voxel1(batch, origin) == V).all()
        assert n27 > max(n27 // 2, 8)
        ctx.map_add(batch, downsample=False)
        ref = np.concatenate([ref, batch])
        st1 = ctx.map_stats()
        assert st1["relinearisations"] == st0["relinearisations"] and st1["incremental_adds"] == st0["incremental_adds"] + 1
        assert st1["slots_used"][1] == st0["slots_used"][1], "the relocation batch was meant to stay inside existing level-1 buckets"
        assert st1["pool_used"][1] >= st0["pool_used"][1] + n27 + n27 // 2, (st0["pool_used"], st1["pool_used"])   # runs moved to fresh room
        _check_both_paths(capi, ctx, oracle, ref, origin, state, scan, sc)
        # 2. new level-1 voxels: a strip beyond the mapped walls
        L = float(sc["L"])
        fresh = (rng.uniform(-1, 1, (400, 3)) * [1.5, 3.0, 0.02] + [L + 4.0, 0.0, 0.5]).astype(np.float32)
        ctx.map_add(fresh, downsample=False)
        ref = np.concatenate([ref, fresh])
        st2 = ctx.map_stats()
        assert st2["slots_used"][1] > st1["slots_used"][1] and st2["relinearisations"] == st0["relinearisations"]
        _check_both_paths(capi, ctx, oracle, ref, origin, state, scan, sc)
        # ... and queries inside the new strip, 1 m above it: level 1 decides them out of buckets made by the insert
        ident = np.zeros(26)
        ident[6] = ident[10] = 1.0
        probe = (fresh[:256] + np.array([0, 0, 0.9], np.float32)).astype(np.float32)
        oi, od, f0, f1 = _fails(oracle, ref, origin, ident, probe)
        assert (f0 & ~f1).sum() > 100
        ctx.scan_set(probe)
        ctx.iterate(ident)
        idx, d2 = ctx.fetch_knn()
        assert np.array_equal(idx, oi) and np.array_equal(_bits(d2), _bits(od))
        # 3. deletions through the down-sampling box rule: re-observed ground
        again = (ref[rng.integers(0, len(ref), 3000)] + rng.normal(0, 0.03, (3000, 3))).astype(np.float32)
        ctx.map_add(again, downsample=True)
        ref2 = oracle.map_add(ref, again, downsample=True)
        assert len(ref2) < len(ref) + len(again)
        ref = ref2
        assert ctx.map_size() == len(ref) and ctx.map_stats()["tombstones"] > 0
        _check_both_paths(capi, ctx, oracle, ref, origin, state, scan, sc)
        # 4. eviction by runs
        blo, bhi = np.array([-4.0, -20.0, -1.0], np.float32), np.array([20.0, 20.0, 9.0], np.float32)
        inside = np.all((ref >= blo) & (ref <= bhi), axis=1)
        assert ctx.map_evict_box(blo, bhi, keep_inside=True) == int((~inside).sum()) and (~inside).sum() > 1000
        ref = ref[inside]
        _check_both_paths(capi, ctx, oracle, ref, origin, state, scan, sc, min_share=0.25)
        # 5. forced re-linearisation, stop-the-world ...
        ctx.map_relinearise()
        assert ctx.map_stats()["relinearisations"] == st0["relinearisations"] + 1
        assert np.array_equal(_bits(ctx.map_fetch()), _bits(ref))
        _check_both_paths(capi, ctx, oracle, ref, origin, state, scan, sc)
        # ... and in the background, with an insert journaled meanwhile and replayed on adoption
        ctx.set_option("async_relinearise_test_delay_ms", 50)
        ctx.map_relinearise_async()
        more = (ref[rng.integers(0, len(ref), 500)] + rng.normal(0, 0.03, (500, 3))).astype(np.float32)
        ctx.map_add(more, downsample=True)
        ref = oracle.map_add(ref, more, downsample=True)
        s = ctx.map_rebuild_status(wait=True)
        assert s["adopted"] == 1 and s["journal"] == 0, s
        assert np.array_equal(_bits(ctx.map_fetch()), _bits(ref))
        _check_both_paths(capi, ctx, oracle, ref, origin, state, scan, sc)


def test_map_stats_account_for_level1(capi, oracle, scene):
    sc = scene
    with capi.Context(capi.default_params(MAX_NUM_ITERS=0)) as ctx:
        ctx.map_build(sc["map_xyz"])
        st = ctx.map_stats()
        assert st["pool_used"][0] > 0 and st["pool_used"][1] > 0 and st["pool_used"][2] > 0
        assert st["slots_used"][1] > 0 and st["slots_cap"][1] >= 2 * st["slots_used"][1]
        assert st["pool_cap"][1] >= st["pool_used"][1]
        # every point lies in 27 level-1 buckets, every run has slack behind it
        assert st["pool_used"][1] >= 27 * len(sc["map_xyz"])
        # bytes: both pools (12-byte points + ids), both tables with their aux records, 2 x 27 back-positions per id
        floor = sum(st["pool_cap"][l] * 16 + st["slots_cap"][l] * 32 for l in (0, 1)) + st["pool_cap"][2] * 16 + st["capacity"] * (2 * 27 * 2 + 4)
        assert st["bytes"] >= floor, (st["bytes"], floor)
        # read-only calls leave the statistics alone
        ctx.scan_set(sc["scan_xyz"])
        ctx.iterate(_off_pose(sc, 1.2))
        ctx.fetch_knn()
        ctx.map_knn(sc["map_xyz"][:64], 5)
        ctx.map_fetch()
        assert ctx.map_stats() == st
