"""GPU tests of lv_map_cluster / lv_map_remove_clusters (lv_cluster.hip) against the scipy statement of the rule in
tests/cluster_ref.py.  The result is a partition with a unique numbering: labels, sizes and C are compared with
np.array_equal, no tolerance, no point left out."""
import ctypes as C
import time

import numpy as np
import pytest
from scipy.spatial import cKDTree

import cluster_ref as cr

pytestmark = pytest.mark.gpu

LV_EINVAL = -1


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
    """500 points each >= 1 m from every other point of the map and from each other (as tests/test_gpu_map_surface.py builds them)."""
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
    return out.astype(np.float32)


@pytest.fixture(scope="module")
def cloud(scene, ghosts):
    xyz = np.concatenate([scene["map_xyz"], ghosts])
    return xyz[np.random.default_rng(9).permutation(len(xyz))]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _hold(out, ref, label=""):
    print(f"{label}: C {out['n_clusters']} (reference {ref['n_clusters']}), largest {list(out['sizes'][:3])}, unlabelled "
          f"{int((out['labels'] < 0).sum())} (reference {int((ref['labels'] < 0).sum())})")
    assert out["n_clusters"] == ref["n_clusters"]
    assert np.array_equal(out["sizes"], ref["sizes"])
    assert np.array_equal(out["labels"], ref["labels"])


@pytest.mark.parametrize("radius", [0.15, 0.3, 0.6, 1.0])
def test_scene_matches_the_reference(capi, cloud, radius):
    # (cell 0.5 m: the level-0 bound of a point lies in [0.5, 1) m, so 0.15 / 0.3 walk the level-0 run, 1.0 the level-2 lists and
    # 0.6 either, point by point)
    with capi.Context() as ctx:
        ctx.map_build(cloud)
        for min_size, max_size in ((1, 0), (10, 0), (1, 40), (5, 200)):
            out = ctx.map_cluster(capi.default_cluster_params(radius=radius, min_size=min_size, max_size=max_size))
            _hold(out, cr.cluster(cloud, radius, min_size, max_size), f"r={radius} sizes {min_size}..{max_size}")
        again = ctx.map_cluster(capi.default_cluster_params(radius=radius, min_size=5, max_size=200))
        assert np.array_equal(out["labels"], again["labels"]) and np.array_equal(out["sizes"], again["sizes"])


def test_a_large_radius(capi, cloud):
    xyz = cloud[:20_000]
    with capi.Context() as ctx:
        ctx.map_build(xyz)
        for min_size in (1, 10):
            _hold(ctx.map_cluster(capi.default_cluster_params(radius=3.0, min_size=min_size)), cr.cluster(xyz, 3.0, min_size), f"r=3 min {min_size}")


def test_optional_outputs(capi, cloud):
    xyz = cloud[:30_000]
    lib = capi.load_library()
    ref = cr.cluster(xyz, 0.3)
    with capi.Context() as ctx:
        ctx.map_build(xyz)
        p = capi.default_cluster_params(radius=0.3)
        n = C.c_size_t(0)
        ctx._check(lib.lv_map_cluster(ctx.h, C.byref(p), None, None, 0, None, 0, C.byref(n)))   # count only
        assert n.value == ref["n_clusters"]
        sizes = np.full(8, 99, np.uint32)
        ctx._check(lib.lv_map_cluster(ctx.h, C.byref(p), None, None, 0, sizes.ctypes.data_as(C.POINTER(C.c_uint32)), 5, None))
        assert np.array_equal(sizes[:5], ref["sizes"][:5]) and np.all(sizes[5:] == 99)


def test_ground_mask_from_the_normals(capi, cloud):
    from limo_velo_amd import cluster

    with capi.Context() as ctx:
        ctx.map_build(cloud)
        normals = ctx.map_normals()["normals"]
        mask = cluster.ground_mask(normals, 15.0)
        assert 0 < mask.sum() < len(cloud)
        for radius in (0.3, 1.0):
            out = ctx.map_cluster(capi.default_cluster_params(radius=radius, min_size=3), mask=mask)
            ref = cr.cluster(cloud, radius, 3, 0, mask)
            _hold(out, ref, f"masked r={radius}")
            assert np.all(out["labels"][mask == 0] == -1)
        b = cluster.boxes(ctx.map_fetch(), out["labels"], out["n_clusters"])
        assert np.array_equal(b["count"], out["sizes"].astype(np.int64))
        assert np.all(b["min"] <= b["centroid"]) and np.all(b["centroid"] <= b["max"])
        # an excluded point links nothing: two blobs joined only through an excluded bridge stay apart
    bridge = np.array([[0, 0, 0], [0.4, 0, 0], [0.8, 0, 0], [1.2, 0, 0], [1.6, 0, 0]], np.float32)
    with capi.Context() as ctx:
        ctx.map_build(bridge)
        out = ctx.map_cluster(capi.default_cluster_params(radius=0.5), mask=[1, 1, 0, 1, 1])
        assert list(out["labels"]) == [0, 0, -1, 1, 1] and list(out["sizes"]) == [2, 2]
        assert list(ctx.map_cluster(capi.default_cluster_params(radius=0.5))["labels"]) == [0] * 5


def test_after_an_eviction_and_a_downsampling_insert(capi, scene, cloud):
    xyz = cloud[:60_000]
    with capi.Context() as ctx:
        ctx.map_build(xyz)
        ctx.map_evict_box(np.array([-1e3, -1e3, -1e3], np.float32), np.array([1e3, 0.0, 1e3], np.float32), keep_inside=False)
        left = ctx.map_fetch()
        assert 0 < len(left) < len(xyz)   # (dead ids: rank != id from here on)
        for radius in (0.3, 1.0):
            _hold(ctx.map_cluster(capi.default_cluster_params(radius=radius, min_size=2)), cr.cluster(left, radius, 2), f"evicted r={radius}")
        mask = (np.arange(len(left)) % 3 != 0).astype(np.uint8)
        _hold(ctx.map_cluster(capi.default_cluster_params(radius=0.3), mask=mask), cr.cluster(left, 0.3, 1, 0, mask), "evicted, masked")
        ctx.map_add(cloud[60_000:75_000] + np.float32(0.013), downsample=True)   # (in flight: the next call settles it)
        out = ctx.map_cluster(capi.default_cluster_params(radius=0.3, min_size=2))
        now = ctx.map_fetch()
        assert len(left) < len(now) <= len(left) + 15_000
        _hold(out, cr.cluster(now, 0.3, 2), "after a down-sampling insert")
        _hold(ctx.map_cluster(capi.default_cluster_params(radius=1.0)), cr.cluster(now, 1.0), "after a down-sampling insert r=1")


def test_degenerate_maps(capi):
    with capi.Context() as ctx:   # an empty map: C = 0, nothing written
        out = ctx.map_cluster()
        assert out["n_clusters"] == 0 and out["labels"].shape == (0,)
        assert ctx.map_remove_clusters(capi.default_cluster_params(min_size=5))["n_removed"] == 0
        ctx.map_build(np.array([[1, 2, 3]], np.float32))   # one point
        out = ctx.map_cluster()
        assert out["n_clusters"] == 1 and list(out["labels"]) == [0] and list(out["sizes"]) == [1]
        assert ctx.map_cluster(capi.default_cluster_params(min_size=2))["n_clusters"] == 0
    rng = np.random.default_rng(5)
    base = rng.uniform(-2, 2, (3000, 3)).astype(np.float32)
    dup = np.concatenate([base, base[:1000], base[:300]])   # exact duplicates are adjacent at any radius
    with capi.Context() as ctx:
        ctx.map_build(dup)
        for radius in (1e-6, 0.1, 0.3):
            _hold(ctx.map_cluster(capi.default_cluster_params(radius=radius)), cr.cluster(dup, radius), f"duplicates r={radius}")
        out = ctx.map_cluster(capi.default_cluster_params(radius=1e-6))
        assert list(out["sizes"][:301]) == [3] * 300 + [2] and out["n_clusters"] == 3000
        ctx.map_build(base[:800])   # (more lists than ids at this radius: every id is walked)
        out = ctx.map_cluster(capi.default_cluster_params(radius=10.0))
        _hold(out, cr.cluster(base[:800], 10.0), "everything in one cluster")
        assert out["n_clusters"] == 1 and list(out["sizes"]) == [800]
    # two points at exactly d2 == radius^2 in f32 (0.5 * 0.5 = 0.25, both exact), and one f32 ulp beyond
    beyond = np.nextafter(np.float32(0.5), np.float32(1))
    assert np.float32(beyond * beyond) > np.float32(0.25)
    pts = np.array([[0, 0, 0], [0.5, 0, 0], [0, 5, 0], [0, 5, beyond]], np.float32)
    with capi.Context() as ctx:
        ctx.map_build(pts)
        out = ctx.map_cluster(capi.default_cluster_params(radius=0.5))
        _hold(out, cr.cluster(pts, 0.5), "the boundary")
        assert list(out["labels"]) == [0, 0, 1, 2]


def test_a_long_chain_in_shuffled_order(capi):
    n, radius = 50_000, 0.5
    t = np.arange(n, dtype=np.float64) * (0.9 * radius)
    # a helix, so that the chain stays inside the voxel range and only successive points are adjacent
    R = 400.0
    pts = np.stack([R * np.cos(t / R), R * np.sin(t / R), t * 0.01], axis=1).astype(np.float32)
    pts = pts[np.random.default_rng(4).permutation(n)]
    ref = cr.cluster(pts, radius)
    assert ref["n_clusters"] == 1
    with capi.Context() as ctx:
        ctx.map_build(pts)
        t0 = time.perf_counter()
        out = ctx.map_cluster(capi.default_cluster_params(radius=radius))
        print(f"chain of {n}: {(time.perf_counter() - t0) * 1e3:.1f} ms")
        _hold(out, ref, "chain")


def _blobs():
    """A wall of 4000 points, three objects of 300 points 2 m in front of it, debris blobs of 1..8 points: (xyz, kind) shuffled;
    kind 0 wall, 1..3 objects, 9 debris."""
    rng = np.random.default_rng(21)
    wall = np.stack([rng.uniform(-10, 10, 4000), np.full(4000, 6.0), rng.uniform(0, 3, 4000)], axis=1)
    objs = [c + rng.uniform(-0.4, 0.4, (300, 3)) for c in ([-5.0, 3.0, 0.5], [0.0, 3.0, 0.5], [5.0, 3.0, 0.5])]
    debris = [np.array([x, -4.0, 1.0]) + rng.uniform(-0.05, 0.05, (1 + i % 8, 3)) for i, x in enumerate(np.linspace(-9.5, 9.5, 20))]
    xyz = np.concatenate([wall] + objs + debris).astype(np.float32)
    kind = np.concatenate([np.zeros(4000), np.repeat([1, 2, 3], 300), np.full(sum(len(d) for d in debris), 9)]).astype(np.int32)
    perm = rng.permutation(len(xyz))
    return xyz[perm], kind[perm]


def test_debris_removal(capi, cloud):
    for xyz, radius, min_size in ((_blobs()[0], 0.4, 10), (cloud[:50_000], 0.3, 4)):
        ref = cr.removed(xyz, radius, min_size)
        assert 0 < ref.sum() < len(xyz)
        with capi.Context() as ctx:
            ctx.map_build(xyz)
            dry = ctx.map_remove_clusters(capi.default_cluster_params(radius=radius, min_size=min_size, max_size=3), dry_run=True)
            assert dry["n_removed"] == 0 and ctx.map_size() == len(xyz)
            assert np.array_equal(dry["flags"].astype(bool), ref)   # (max_size is ignored in this mode)
            got = ctx.map_remove_clusters(capi.default_cluster_params(radius=radius, min_size=min_size))
            assert got["n_removed"] == int(ref.sum()) and np.array_equal(got["flags"].astype(bool), ref)
            assert np.array_equal(_bits(ctx.map_fetch()), _bits(xyz[~ref]))   # the survivors, in order
            # the map still serves: a second pass finds nothing, the clusters are those of the survivors
            assert ctx.map_remove_clusters(capi.default_cluster_params(radius=radius, min_size=min_size))["n_removed"] == 0
            _hold(ctx.map_cluster(capi.default_cluster_params(radius=radius)), cr.cluster(xyz[~ref], radius), "after the debris left")


def test_debris_helper_and_mask(capi):
    from limo_velo_amd import cluster

    xyz, kind = _blobs()
    mask = (kind != 9) | (np.arange(len(xyz)) % 2 == 0)   # half of the debris is excluded: it is never removed
    ref = cr.removed(xyz, 0.4, 10, mask=mask)
    with capi.Context() as ctx:
        ctx.map_build(xyz)
        got = cluster.remove_debris(ctx, 0.4, 10, mask=mask)
        assert np.array_equal(got["flags"].astype(bool), ref) and not np.any(got["flags"][~mask])
        assert np.array_equal(_bits(ctx.map_fetch()), _bits(xyz[~ref]))


def test_seeded_removal_takes_the_object_whole(capi):
    xyz, kind = _blobs()
    radius = 0.4
    assert cr.cluster(xyz, radius, 100)["n_clusters"] == 4   # the wall and the three objects
    seeds = np.zeros(len(xyz), np.uint8)
    seeds[np.flatnonzero(kind == 2)[:3]] = 1     # three hits on object 2
    seeds[np.flatnonzero(kind == 0)[:5]] = 1     # and five on the wall
    prm = capi.default_cluster_params(radius=radius, min_size=1, max_size=1000)
    ref = cr.removed(xyz, radius, 1, 1000, seeds=seeds)
    assert np.array_equal(ref, kind == 2)        # the object whole; the wall (4000 > max_size) stays
    with capi.Context() as ctx:
        ctx.map_build(xyz)
        dry = ctx.map_remove_clusters(prm, seeds=seeds, dry_run=True)
        assert dry["n_removed"] == 0 and np.array_equal(dry["flags"].astype(bool), ref)
        only_wall = np.where(kind == 0, seeds, 0)
        none = ctx.map_remove_clusters(prm, seeds=only_wall)   # seeds on a component above max_size: nothing goes
        assert none["n_removed"] == 0 and not none["flags"].any() and ctx.map_size() == len(xyz)
        # an excluded seed seeds nothing, and an excluded point never leaves
        mask = np.ones(len(xyz), np.uint8)
        mask[np.flatnonzero(kind == 2)[:3]] = 0
        masked = ctx.map_remove_clusters(prm, mask=mask, seeds=seeds, dry_run=True)
        assert np.array_equal(masked["flags"].astype(bool), cr.removed(xyz, radius, 1, 1000, mask=mask, seeds=seeds))
        assert not masked["flags"].any()
        mask = np.ones(len(xyz), np.uint8)
        mask[np.flatnonzero(kind == 2)[10:20]] = 0
        refm = cr.removed(xyz, radius, 1, 1000, mask=mask, seeds=seeds)
        masked = ctx.map_remove_clusters(prm, mask=mask, seeds=seeds, dry_run=True)
        assert np.array_equal(masked["flags"].astype(bool), refm) and not np.any(masked["flags"][mask == 0]) and refm.sum() > 0
        got = ctx.map_remove_clusters(prm, seeds=seeds)
        assert got["n_removed"] == 300 and np.array_equal(got["flags"].astype(bool), ref)
        assert np.array_equal(_bits(ctx.map_fetch()), _bits(xyz[~ref]))
        # without an upper limit the seeded wall goes too
        left, seeds_left = xyz[~ref], seeds[~ref]
        got = ctx.map_remove_clusters(capi.default_cluster_params(radius=radius, min_size=1, max_size=0), seeds=seeds_left)
        assert np.array_equal(got["flags"].astype(bool), cr.removed(left, radius, 1, 0, seeds=seeds_left)) and got["n_removed"] == 4000


def test_removal_during_a_background_rebuild(capi, cloud, ghosts):
    xyz = cloud[:60_000]

    def run(ctx, background):
        ctx.set_option("async_relinearise", 1 if background else 0)
        ctx.map_build(xyz)
        ctx.map_evict_box(np.array([-1e3, -1e3, -1e3], np.float32), np.array([1e3, 0.0, 1e3], np.float32), keep_inside=False)
        if background:
            ctx.set_option("async_relinearise_test_delay_ms", 400)
            ctx.map_relinearise_async()
            t0 = time.monotonic()
            while ctx.map_rebuild_status()["state"] in (4, 5) and time.monotonic() - t0 < 10:   # until the snapshot is taken
                ctx.map_size()
                time.sleep(0.001)
            assert ctx.map_rebuild_status()["state"] == 1
        ctx.map_add(ghosts[:100] + np.float32(0.02))   # (journaled for the copy)
        running = ctx.map_rebuild_status()["state"]
        before = ctx.map_fetch()
        labels = ctx.map_cluster(capi.default_cluster_params(radius=0.3))   # (read-only: reads the active store, no wait)
        mask = (np.arange(len(before)) % 7 != 0).astype(np.uint8)
        n0 = ctx.map_remove_clusters(capi.default_cluster_params(radius=0.3, min_size=4), mask=mask)
        st = ctx.map_rebuild_status()
        seeds = np.zeros(ctx.map_size(), np.uint8)
        seeds[::500] = 1
        n1 = ctx.map_remove_clusters(capi.default_cluster_params(radius=0.3, min_size=1, max_size=60), seeds=seeds)
        return ctx.map_fetch(), before, labels, running, st, (n0, n1), mask

    with capi.Context() as a:
        fa, ba, la, running, sa, na, mask = run(a, True)
    with capi.Context() as b:
        fb, bb, lb, _, _, nb, _ = run(b, False)
    # the removal waited for the rebuild to land (it was still running before it), and nothing was lost on the way
    assert running == 1 and sa["adopted"] >= 1 and sa["state"] == 0, (running, sa)
    assert np.array_equal(_bits(ba), _bits(bb)) and np.array_equal(la["labels"], lb["labels"])
    assert na[0]["n_removed"] == nb[0]["n_removed"] > 0 and na[1]["n_removed"] == nb[1]["n_removed"] > 0
    assert np.array_equal(na[0]["flags"], nb[0]["flags"]) and np.array_equal(na[1]["flags"], nb[1]["flags"])
    assert np.array_equal(na[0]["flags"].astype(bool), cr.removed(ba, 0.3, 4, mask=mask))
    assert np.array_equal(_bits(fa), _bits(fb))


def test_dynamic_objects_helper(capi):
    """remove_dynamic_objects: a box standing in an empty room that a later sweep sees through goes whole, far side included."""
    from limo_velo_amd import cluster

    rng = np.random.default_rng(8)
    n = 20_000
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    shell = (d * 20.0).astype(np.float32)                                # the room: a sphere of 20 m around the sensor
    box = (np.array([5.0, 0.0, 0.0]) + rng.uniform(-0.5, 0.5, (2000, 3))).astype(np.float32)
    xyz = np.concatenate([shell, box])
    with capi.Context() as ctx:
        ctx.map_build(xyz)
        views = [(np.eye(3, dtype=np.float32), np.zeros(3, np.float32), shell)]   # a sweep that sees the room, not the box
        vis = capi.default_visibility_params(width=360, height=90, v_min_deg=-89.0, v_max_deg=89.0, window=2)
        _, hits = ctx.map_remove_dynamic(views, vis, dry_run=True)
        assert 0 < hits[n:].sum() and hits[:n].sum() == 0
        got = cluster.remove_dynamic_objects(ctx, views, vis, radius=0.3, max_size=5000)
        assert np.array_equal(got["hits"], hits)
        # the box is one component at 0.3 m (2000 points in 1 m^3), the shell's points are further apart than that from it
        assert got["n_clusters"] == 2000 and ctx.map_size() == n
        assert np.array_equal(_bits(ctx.map_fetch()), _bits(shell))


def test_invalid_arguments_change_nothing(capi, cloud):
    xyz = cloud[:20_000]
    lib = capi.load_library()
    nan, inf = float("nan"), float("inf")
    bad = [dict(radius=0.0), dict(radius=-1.0), dict(radius=nan), dict(radius=inf), dict(min_size=0)]
    with capi.Context() as ctx:
        ctx.map_build(xyz)
        m = len(xyz)
        labels = np.full(m, 7, np.int32)
        fl = np.full(m, 9, np.uint8)
        n = C.c_size_t(123)
        lp, fp = labels.ctypes.data_as(C.POINTER(C.c_int32)), fl.ctypes.data_as(C.POINTER(C.c_uint8))
        for kw in bad:
            p = capi.default_cluster_params(**kw)
            assert lib.lv_map_cluster(ctx.h, C.byref(p), None, lp, m, None, 0, C.byref(n)) == LV_EINVAL, kw
            assert lib.lv_map_remove_clusters(ctx.h, C.byref(p), None, None, fp, C.byref(n)) == LV_EINVAL, kw
            assert n.value == 123   # (nothing written)
        p = capi.default_cluster_params()
        assert lib.lv_map_cluster(ctx.h, None, None, lp, m, None, 0, C.byref(n)) == LV_EINVAL
        assert lib.lv_map_remove_clusters(ctx.h, None, None, None, fp, C.byref(n)) == LV_EINVAL
        assert lib.lv_map_cluster(ctx.h, C.byref(p), None, lp, m - 1, None, 0, C.byref(n)) == LV_EINVAL   # capacity < m
        assert n.value == 123 and np.all(labels == 7) and np.all(fl == 9) and ctx.map_size() == m
        assert np.array_equal(_bits(ctx.map_fetch()), _bits(xyz))
