"""GPU tests across the map tools: lv_map_knn, lv_map_normals, lv_map_radius_search, lv_map_remove_outliers and lv_map_cluster walk
the same k-NN ladder and the same fixed-radius sources (lv_query_dev.hpp: knn_ladder, radius_source / stream_radius), so on one map
they must see the same neighbours on every rung and every source, and a removal must be counted the same way whoever asks for it.

The map: 3 000 points, 600 uniform in each of five cubes centred on the origin (edges 4, 10, 25, 60, 150 m), so that the 5th
neighbour of a point lies below the level-0 bound, inside each of the ladder's four radii bands or beyond them all.  The reference
is one brute-force table of f32 calc_dist keys (d2 bits << 32 | index), computed once and shared.

Removal accounting keeps the 3 000-point map (a map removed whole is rebuilt empty, which sets the tombstone count back to zero on
every path: nothing would be compared).  On it the outlier rule takes the sparse outside and a box a convex inside, so no single
box holds exactly an outlier rule's set: for radius 40 and fewer than 30 neighbours, the 200 points of the test, the bounding box
of the set holds 2 799 other points (asserted below).  The set is therefore the outlier rule's, the mask marks exactly it, and the
box removal takes it with one degenerate box [p, p] per point, each of which encloses exactly its point."""
import numpy as np
import pytest

import cluster_ref as cr

pytestmark = pytest.mark.gpu

SEED = 20261018
NONE = np.uint32(0xFFFFFFFF)
ALL = np.uint64(0xFFFFFFFF)


@pytest.fixture(scope="module")
def capi(lv):
    from limo_velo_amd import capi as c

    return c


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def cloud():
    rng = np.random.default_rng(SEED)
    pts = np.concatenate([rng.uniform(-e / 2, e / 2, (600, 3)) for e in (4, 10, 25, 60, 150)]).astype(np.float32)
    return np.ascontiguousarray(pts[rng.permutation(len(pts))])


@pytest.fixture(scope="module")
def table(cloud):
    """keys [m, m] uint64, every row ascending: (d2 bits << 32 | index) of every map point against the row's point, d2 in
    calc_dist's f32 order ((dx^2 + dy^2) + dz^2, unfused).  Read-only."""
    d = cloud[:, None, :] - cloud[None, :, :]
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    keys = (d2.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.arange(len(cloud), dtype=np.uint64)[None, :]
    keys.sort(axis=1)
    keys.setflags(write=False)
    return keys


def _key_d2(keys):
    return (keys >> np.uint64(32)).astype(np.uint32).view(np.float32)


def _ref_knn(table, k, max_dist):
    md = np.float32(max_dist)
    key = table[:, :k]
    d2 = _key_d2(key)
    ok = d2 <= md * md
    idx = np.where(ok, (key & ALL).astype(np.uint32), NONE)
    return idx, np.where(ok, d2, np.float32(np.inf)), ok.sum(axis=1).astype(np.int32)


def _ref_radius(table, r):
    """(offsets, idx, d2) in CSR, every list ascending by index; counts [m] with the point itself."""
    hit = _key_d2(table) <= np.float32(r) * np.float32(r)
    cnt = hit.sum(axis=1)
    rows = np.repeat(np.arange(len(table)), cnt)
    key = table[hit]                       # row-major: each row's hits, ascending (d2, index)
    idx = (key & ALL).astype(np.uint32)
    order = np.lexsort((idx, rows))        # ... put into ascending index inside the row
    off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.uint64)
    return off, idx[order], _key_d2(key)[order], cnt


@pytest.fixture(scope="module")
def ctx(capi, cloud):
    c = capi.Context()
    c.map_build(cloud)   # (the default 0.5 m voxel)
    yield c
    c.close()


def test_every_rung_is_taken(table):
    """The 5th neighbour (the point itself included) below the smallest level-0 bound, inside each band of the four radii
    ([0.5, 1), [1, 2), [2, 4), [4, 8) m) and beyond the last: at least 100 points each, so no rung of the ladder goes untested."""
    d5 = np.sqrt(_key_d2(table[:, 4]).astype(np.float64))
    bands = [(d5 < 0.49).sum()] + [((d5 >= lo) & (d5 < 2 * lo)).sum() for lo in (0.5, 1.0, 2.0, 4.0)] + [(d5 >= 8.0).sum()]
    print("points per band:", [int(b) for b in bands])
    assert min(bands) >= 100


@pytest.mark.parametrize("max_dist", [2.0, 200.0])
@pytest.mark.parametrize("k", [5, 10])
def test_ladder(capi, ctx, cloud, table, k, max_dist):
    wi, wd, wf = _ref_knn(table, k, max_dist)
    gi, gd, gf = ctx.map_knn(cloud, k, max_dist=max_dist)
    assert np.array_equal(gi, wi)
    assert np.array_equal(_bits(gd), _bits(wd))
    assert np.array_equal(gf, wf)
    out = ctx.map_normals(capi.default_surface_params(k=k, max_dist=max_dist))
    assert np.array_equal(out["n_used"], wf)
    # the mean distance to the others: sqrt in f64, summed in neighbour order (one vectorised add per neighbour), / (n - 1), to f32
    s = np.zeros(len(cloud))
    for j in range(k):
        s = s + np.where(j < wf, np.sqrt(np.where(j < wf, wd[:, j], np.float32(0)).astype(np.float64)), 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        mean = np.where(wf > 1, (s / (wf - 1)).astype(np.float32), np.float32(np.inf))
    print(f"k {k} max_dist {max_dist}: found {np.bincount(wf, minlength=k + 1).tolist()}")
    assert np.array_equal(_bits(out["mean_dist"]), _bits(mean))


@pytest.mark.parametrize("r", [0.3, 1.5, 40.0])
def test_sources(capi, ctx, cloud, table, r):
    """0.3: under every level-0 bound, the run; 1.5: above them, at most 5^3 lists < 3 000 ids, the level-2 list box; 40: about
    43^3 lists, more than the ids, every id."""
    wo, wi, wd, cnt = _ref_radius(table, r)
    off, idx, d2 = ctx.map_radius(cloud, r)
    assert np.array_equal(off, wo)
    assert np.array_equal(idx, wi)
    assert np.array_equal(_bits(d2), _bits(wd))
    for n in (1, 3):
        _, flags, _ = ctx.map_remove_outliers(capi.default_outlier_params(mode=1, radius=r, min_neighbours=n), dry_run=True)
        assert np.array_equal(flags != 0, cnt - 1 < n)
    ref = cr.cluster(cloud, r)
    out = ctx.map_cluster(capi.default_cluster_params(radius=r))
    print(f"r {r}: {int(wo[-1])} pairs, {ref['n_clusters']} clusters")
    assert out["n_clusters"] == ref["n_clusters"]
    assert np.array_equal(out["sizes"], ref["sizes"])
    assert np.array_equal(out["labels"], ref["labels"])


def test_removal_accounting(capi, cloud, table):
    """The same 200 points leave three maps by lv_map_evict_box, lv_map_remove_clusters and lv_map_remove_outliers: the maps agree
    afterwards and lv_map_get_stats().tombstones rose by the same number on all three."""
    r, n = 40.0, 30
    cnt = _ref_radius(table, r)[3] - 1
    gone = cnt < n
    assert gone.sum() == 200
    inside = ((cloud >= cloud[gone].min(axis=0)) & (cloud <= cloud[gone].max(axis=0))).all(axis=1)
    assert (inside & ~gone).sum() == 2799   # (why the box removal goes point by point: module docstring)
    assert np.array_equal(cr.removed(cloud, r, 201, 0, gone), gone)   # (no component of the marked points reaches 201)
    left, rose, knn = [], [], []

    def box(c):
        for p in cloud[gone]:
            assert c.map_evict_box(p, p, keep_inside=False) == 1
        return 200

    def clusters(c):
        out = c.map_remove_clusters(capi.default_cluster_params(radius=r, min_size=201), mask=gone)
        assert np.array_equal(out["flags"] != 0, gone)
        return out["n_removed"]

    def outliers(c):
        nr, flags, _ = c.map_remove_outliers(capi.default_outlier_params(mode=1, radius=r, min_neighbours=n))
        assert np.array_equal(flags != 0, gone)
        return nr

    for remove in (box, clusters, outliers):
        with capi.Context() as c:
            c.map_build(cloud)
            t0 = c.map_stats()["tombstones"]
            assert remove(c) == 200
            assert c.map_size() == len(cloud) - 200
            rose.append(c.map_stats()["tombstones"] - t0)
            left.append(c.map_fetch())
            knn.append(c.map_knn(cloud, 5))
    print("tombstones rose by", rose)
    assert np.array_equal(_bits(left[0]), _bits(cloud[~gone]))
    for i in (1, 2):
        assert np.array_equal(_bits(left[i]), _bits(left[0]))
        assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(knn[i], knn[0]))
    assert rose[0] == rose[1] == rose[2] > 0
