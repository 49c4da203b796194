"""GPU tests of lv_map_planes (lv_planes.hip) against the numpy statement of the rule in tests/planes_ref.py.  The result is
exactly defined: labels, counts and indices are compared with np.array_equal, normals, anchors, d and rms by their bits; no
tolerance, no point left out, no case skipped.  The room and every small map here are chosen so that the reference alone decides
each case (test_the_reference_decides_the_room runs without the library's answer)."""
import ctypes as C
import math
import time

import numpy as np
import pytest

import plane_cases as pc
import planes_ref as pr

pytestmark = pytest.mark.gpu

LV_EINVAL = -1
F = np.float32
RAMP_DEG = 20.0
ROOM = dict(distance=0.05, iterations=256, min_inliers=1000)   # (any 0.1 m slab of the room holds some 500 points of walls and clutter)


@pytest.fixture(scope="module")
def capi(lv):
    from limo_velo_amd import capi as c

    return c


def make_room(seed=3):
    """About 20 k points, shuffled: a floor, two walls, a ramp tilted by RAMP_DEG about y, a table top, 10 % clutter; 5 mm noise.
    (xyz [m, 3] f32, kind [m]: 0 floor, 1 wall x = 0, 2 wall y = 0, 3 ramp, 4 table top, 5 clutter)"""
    rng = np.random.default_rng(seed)
    parts = []

    def add(kind, pts):
        parts.append((np.full(len(pts), kind), pts))

    n = 8000
    add(0, np.column_stack([rng.uniform(0, 10, n), rng.uniform(0, 8, n), np.zeros(n)]))
    n = 3500
    add(1, np.column_stack([np.zeros(n), rng.uniform(0, 8, n), rng.uniform(0, 3, n)]))
    add(2, np.column_stack([rng.uniform(0, 10, n), np.zeros(n), rng.uniform(0, 3, n)]))
    n = 2500
    x = rng.uniform(5, 8, n)
    add(3, np.column_stack([x, rng.uniform(2, 5, n), 0.3 + math.tan(math.radians(RAMP_DEG)) * (x - 5.0)]))
    n = 600
    add(4, np.column_stack([rng.uniform(1, 2.2, n), rng.uniform(5, 6.2, n), np.full(n, 0.75)]))
    n = 2000
    add(5, np.column_stack([rng.uniform(0, 10, n), rng.uniform(0, 8, n), rng.uniform(0, 3, n)]))
    kind = np.concatenate([k for k, _ in parts])
    xyz = np.concatenate([p for _, p in parts])
    xyz[kind != 5] += rng.normal(size=(int((kind != 5).sum()), 3)) * 0.005
    order = rng.permutation(len(xyz))
    return xyz[order].astype(F), kind[order]


@pytest.fixture(scope="module")
def room():
    return make_room()


@pytest.fixture(scope="module")
def room_ctx(capi, room):
    """one context that holds the room for the read-only tests"""
    with capi.Context() as ctx:
        ctx.map_build(room[0])
        assert np.array_equal(pr.b32(ctx.map_fetch()), pr.b32(room[0]))   # (map order is the order given)
        yield ctx


_REF = {}


def room_ref(room, **kw):
    """the reference on the room, computed once per parameter set and shared"""
    key = tuple(sorted((k, tuple(v) if isinstance(v, (list, tuple)) else v) for k, v in kw.items()))
    if key not in _REF:
        _REF[key] = pr.segment(room[0], {**ROOM, **kw})
    return _REF[key]


def hold(out, ref, label=""):
    print(f"{label}: P {out['n_planes']} (reference {ref['n_planes']}), inliers {[int(p['inliers']) for p in out['planes']]} "
          f"(reference {[p['inliers'] for p in ref['planes']]}), hypotheses {[int(p['hypothesis']) for p in out['planes']]}")
    assert out["n_planes"] == ref["n_planes"]
    for got, want in zip(out["planes"], ref["planes"]):
        for k in ("inliers", "support", "hypothesis", "candidates", "n_fit", "flags"):
            assert int(got[k]) == want[k], (label, k, int(got[k]), want[k])
        assert np.array_equal(pr.b32(got["normal"]), pr.b32(want["normal"])), (label, got["normal"], want["normal"])
        assert np.array_equal(pr.b32(got["anchor"]), pr.b32(want["anchor"])), (label, got["anchor"], want["anchor"])
        assert pr.b64(got["d"])[0] == pr.b64(want["d"])[0] and pr.b64(got["rms"])[0] == pr.b64(want["rms"])[0], (label, got["d"], want["d"], got["rms"], want["rms"])
    assert np.array_equal(out["labels"], ref["labels"])


def planes_of(capi, ctx, mask=None, **kw):
    return ctx.map_planes(capi.default_plane_params(**kw), mask=mask)


def share(labels, kind, k, label):
    """the fraction of the points of kind k that carry the label"""
    return float((labels[kind == k] == label).mean())


# ---- the room: the reference alone first
def test_the_reference_decides_the_room(room):
    """Without the library: the room gives the reference something to decide in every case the GPU tests compare."""
    xyz, kind = room
    assert 19_000 <= len(xyz) <= 21_000 and pr.degenerate(xyz) is None
    one = room_ref(room, max_planes=1)
    assert one["n_planes"] == 1 and share(one["labels"], kind, 0, 0) > 0.99 and abs(float(one["planes"][0]["normal"][2])) > 0.999
    four = room_ref(room, max_planes=4)
    assert four["n_planes"] == 4
    owners = [int(np.bincount(kind[four["labels"] == r]).argmax()) for r in range(4)]
    assert sorted(owners) == [0, 1, 2, 3]                              # floor, both walls and the ramp, each a plane of its own
    assert all(p["flags"] == 1 and p["n_fit"] == p["support"] and 0.003 < p["rms"] < 0.02 for p in four["planes"])
    raw = room_ref(room, max_planes=4, refine=0)
    assert raw["n_planes"] == 4 and all(p["flags"] == 0 and p["n_fit"] == 0 and math.isnan(p["rms"]) for p in raw["planes"])
    assert any(not np.array_equal(a["normal"], b["normal"]) for a, b in zip(raw["planes"], four["planes"]))   # (the refit moves the plane)
    other = room_ref(room, max_planes=4, seed=12345)
    assert [p["hypothesis"] for p in other["planes"]] != [p["hypothesis"] for p in four["planes"]]
    # the constraints on both sides of the ramp's tilt
    z = (0.0, 0.0, 1.0)
    lo = room_ref(room, max_planes=3, constraint=1, axis=z, max_angle=math.radians(RAMP_DEG - 5))
    hi = room_ref(room, max_planes=3, constraint=1, axis=z, max_angle=math.radians(RAMP_DEG + 5))
    assert [int(np.bincount(kind[lo["labels"] == r]).argmax()) for r in range(lo["n_planes"])] == [0, 4]        # floor, table top; no ramp
    assert [int(np.bincount(kind[hi["labels"] == r]).argmax()) for r in range(hi["n_planes"])] == [0, 3]        # the ramp is admitted
    assert all(p["normal"][2] > 0 for p in hi["planes"])                                                           # towards the axis
    lo = room_ref(room, max_planes=3, constraint=2, axis=z, max_angle=math.radians(90 - RAMP_DEG - 5))
    hi = room_ref(room, max_planes=3, constraint=2, axis=z, max_angle=math.radians(90 - RAMP_DEG + 5))
    assert sorted(int(np.bincount(kind[lo["labels"] == r]).argmax()) for r in range(lo["n_planes"])) == [1, 2]  # the walls only
    assert sorted(int(np.bincount(kind[hi["labels"] == r]).argmax()) for r in range(hi["n_planes"])) == [1, 2, 3]


@pytest.mark.parametrize("refine", [1, 0])
@pytest.mark.parametrize("seed", [0, 12345])
@pytest.mark.parametrize("max_planes", [1, 4])
def test_room(capi, room, room_ctx, max_planes, seed, refine):
    kw = dict(max_planes=max_planes, seed=seed, refine=refine)
    hold(planes_of(capi, room_ctx, **ROOM, **kw), room_ref(room, **kw), f"room {kw}")


@pytest.mark.parametrize("constraint,angle_deg", [(1, RAMP_DEG - 5), (1, RAMP_DEG + 5), (2, 90 - RAMP_DEG - 5), (2, 90 - RAMP_DEG + 5)])
def test_room_constraints(capi, room, room_ctx, constraint, angle_deg):
    kw = dict(max_planes=3, constraint=constraint, axis=(0.0, 0.0, 1.0), max_angle=math.radians(angle_deg))
    hold(planes_of(capi, room_ctx, **ROOM, **kw), room_ref(room, **kw), f"constraint {constraint} at {angle_deg} deg")
    kw = dict(max_planes=2, constraint=constraint, axis=(0.1, -0.2, -3.0), max_angle=math.radians(angle_deg), refine=0)   # (an axis to normalise, pointing down)
    hold(planes_of(capi, room_ctx, **ROOM, **kw), room_ref(room, **kw), f"constraint {constraint}, -z axis")


def test_repeat_call_is_equal(capi, room_ctx):
    a = planes_of(capi, room_ctx, **ROOM, max_planes=4)
    b = planes_of(capi, room_ctx, **ROOM, max_planes=4)
    assert np.array_equal(a["labels"], b["labels"]) and a["planes"].tobytes() == b["planes"].tobytes()


# ---- edge sizes: around the wavefront, the hypothesis chunk and the candidate tile of the scoring kernel
def _slab(n, seed):
    """n points of a noisy plane z = 0.1 x - 0.2 y with a third of them scattered off it"""
    rng = np.random.default_rng(seed)
    xy = rng.uniform(-5, 5, (n, 2))
    z = 0.1 * xy[:, 0] - 0.2 * xy[:, 1] + rng.normal(size=n) * 0.01
    z[::3] += rng.uniform(-2, 2, len(z[::3]))
    return np.column_stack([xy, z]).astype(F)


def test_edge_sizes(capi):
    tile, chunk = capi.PLANE_TILE, capi.PLANE_CHUNK
    for n in (3, 63, 64, 65, 257, tile - 1, tile, tile + 1):
        xyz = _slab(n, n)
        with capi.Context() as ctx:
            ctx.map_build(xyz)
            for K in (1, 63, 65, chunk + 1):
                kw = dict(distance=0.03, iterations=K, max_planes=2, min_inliers=3, seed=n + K)
                hold(planes_of(capi, ctx, **kw), pr.segment(xyz, kw), f"n {n} K {K}")


# ---- ties go to the lower h
def test_ties_go_to_the_lower_hypothesis(capi):
    # an exact lattice in the plane z = 0 and a few points off it: every valid hypothesis drawn from the lattice counts the whole
    # lattice.  The seed is chosen on the reference's own counts: hypothesis 0 must not be among the winners.
    g = np.arange(4, dtype=np.float64)
    lattice = np.array([[x, y, 0.0] for x in g for y in g])
    xyz = np.concatenate([lattice, [[0.5, 0.5, 1.0], [1.5, 2.5, -2.0], [2.5, 0.5, 3.0]]]).astype(F)
    q = pr.resolve(dict(distance=0.01, iterations=32, min_inliers=3, refine=0))
    for seed in range(200):
        q["seed"] = seed
        _, valid, _, _, cnt = pr.round_counts(xyz, q, 0)
        top = np.flatnonzero(cnt == cnt.max())
        if len(top) >= 2 and top[0] >= 2 and cnt.max() == 16 and valid[:top[0]].any():
            break
    else:
        raise AssertionError("no seed gives a tie behind a valid, smaller hypothesis")
    kw = dict(distance=0.01, iterations=32, min_inliers=3, refine=0, seed=seed)
    ref = pr.segment(xyz, kw)
    assert ref["planes"][0]["hypothesis"] == int(top[0]) and ref["planes"][0]["support"] == 16
    with capi.Context() as ctx:
        ctx.map_build(xyz)
        hold(planes_of(capi, ctx, **kw), ref, f"ties {list(top)}")


# ---- the threshold: |s| == distance is inside, one ulp beyond is outside
def test_threshold(capi):
    rng = np.random.default_rng(21)
    d = F(0.1)
    up = np.nextafter(d, F(1))
    base = np.column_stack([rng.integers(-20, 21, (400, 2)), np.zeros(400)])            # exact: every hypothesis on it is z = 0
    edge = np.column_stack([rng.integers(-20, 21, (80, 2)), np.tile([d, -d, up, -up], 20)])
    xyz = np.concatenate([base, edge]).astype(F)
    xyz = xyz[rng.permutation(len(xyz))]
    kw = dict(distance=float(d), iterations=64, min_inliers=100, refine=0)
    ref = pr.segment(xyz, kw)
    at, beyond = np.abs(xyz[:, 2]) == d, np.abs(xyz[:, 2]) == up
    assert at.sum() == 40 and beyond.sum() == 40
    assert ref["n_planes"] == 1 and np.array_equal(np.abs(ref["planes"][0]["normal"]), [0, 0, 1])
    assert np.all(ref["labels"][at] == 0) and np.all(ref["labels"][beyond] == -1) and ref["planes"][0]["inliers"] == 440
    with capi.Context() as ctx:
        ctx.map_build(xyz)
        hold(planes_of(capi, ctx, **kw), ref, "threshold")


# ---- degenerate inputs
def test_degenerate_maps(capi):
    t = np.arange(300, dtype=np.float64)[:, None]
    line = (np.array([[1.0, -2.0, 0.5]]) + t * np.array([[0.25, 0.5, 0.75]])).astype(F)
    dup = np.tile(np.array([[1.5, -2.5, 3.0]], F), (300, 1))
    assert pr.degenerate(line) == "collinear" and pr.degenerate(dup) == "duplicate"
    for xyz in (line, dup):
        kw = dict(iterations=128, min_inliers=3)
        ref = pr.segment(xyz, kw)
        assert ref["n_planes"] == 0 and np.all(ref["labels"] == -1)
        with capi.Context() as ctx:
            ctx.map_build(xyz)
            assert ctx.map_size() == 300
            hold(planes_of(capi, ctx, **kw), ref, pr.degenerate(xyz))
    with capi.Context() as ctx:   # an empty map: P = 0, nothing written
        out = ctx.map_planes()
        assert out["n_planes"] == 0 and out["labels"].shape == (0,)


def test_min_inliers_above_the_best_support(capi, room, room_ctx):
    best = room_ref(room, max_planes=1)["planes"][0]["support"]
    for min_inliers, P in ((best, 1), (best + 1, 0)):
        kw = {**ROOM, "max_planes": 4, "min_inliers": min_inliers}
        ref = pr.segment(room[0], kw)
        assert min(ref["n_planes"], 1) == P
        hold(planes_of(capi, room_ctx, **kw), ref, f"min_inliers {min_inliers}")


# ---- a mask, and dead ids
def test_mask_and_dead_ids(capi, room):
    xyz, kind = room
    with capi.Context() as ctx:
        ctx.map_build(xyz)
        mask = ((kind != 0) & (np.arange(len(xyz)) % 5 != 0)).astype(np.uint8)   # without the floor, and a stride of excluded points
        kw = {**ROOM, "max_planes": 3}
        ref = pr.segment(xyz, kw, mask)
        out = planes_of(capi, ctx, mask=mask, **kw)
        hold(out, ref, "masked")
        assert np.all(out["labels"][mask == 0] == -1) and ref["n_planes"] == 3
        ctx.map_evict_box(np.array([-1e3, -1e3, -1e3], F), np.array([1e3, 4.0, 1e3], F), keep_inside=False)
        left = ctx.map_fetch()
        assert 0 < len(left) < len(xyz) and len(left) == ctx.map_size()   # (dead ids: rank != id from here on)
        hold(planes_of(capi, ctx, **kw), pr.segment(left, kw), "evicted")
        mask = (np.arange(len(left)) % 3 != 0).astype(np.uint8)
        hold(planes_of(capi, ctx, mask=mask, **kw), pr.segment(left, kw, mask), "evicted, masked")


# ---- a map 30 km from the origin whose floor reaches beyond the refit's quantised range
def test_far_offset(capi):
    rng = np.random.default_rng(31)
    n = 3000
    near = np.column_stack([30000.0 + rng.uniform(-20, 20, n), 30000.0 + rng.uniform(-20, 20, n), rng.normal(size=n) * 0.004])
    far = np.column_stack([30000.0 - 17000.0 + rng.uniform(-20, 20, n // 3), 30000.0 + rng.uniform(-20, 20, n // 3), rng.normal(size=n // 3) * 0.004])
    junk = np.column_stack([30000.0 + rng.uniform(-20, 20, 300), 30000.0 + rng.uniform(-20, 20, 300), rng.uniform(0.5, 3, 300)])
    xyz = np.concatenate([near, far, junk]).astype(F)
    xyz = xyz[rng.permutation(len(xyz))]
    kw = dict(distance=0.05, iterations=128, min_inliers=100)
    ref = pr.segment(xyz, kw)
    p = ref["planes"][0]
    assert ref["n_planes"] == 1 and p["flags"] == 1 and 0 < p["n_fit"] < p["support"]   # 17 km > 2^22 / 256 m: one patch is left out of the sums
    assert p["support"] == n + n // 3 and p["n_fit"] in (n, n // 3)
    with capi.Context() as ctx:
        ctx.map_build(xyz)
        assert np.array_equal(pr.b32(ctx.map_fetch()), pr.b32(xyz))
        hold(planes_of(capi, ctx, **kw), ref, "far offset")


# ---- optional outputs and refusals
def test_optional_outputs(capi, room, room_ctx):
    lib, ctx = capi.load_library(), room_ctx
    m = len(room[0])
    ref = room_ref(room, max_planes=4)
    p = capi.default_plane_params(**ROOM, max_planes=4)
    n = C.c_size_t(99)
    ctx._check(lib.lv_map_planes(ctx.h, C.byref(p), None, None, 0, None, 0, C.byref(n)))   # count only
    assert n.value == 4
    ctx._check(lib.lv_map_planes(ctx.h, C.byref(p), None, None, 0, None, 0, None))         # nothing asked for
    planes = np.zeros(4, capi.PLANE_DTYPE)
    planes["inliers"] = 77
    ctx._check(lib.lv_map_planes(ctx.h, C.byref(p), None, None, 0, planes.ctypes.data_as(C.POINTER(capi.Plane)), 2, C.byref(n)))
    assert n.value == 4 and [int(v) for v in planes["inliers"]] == [ref["planes"][0]["inliers"], ref["planes"][1]["inliers"], 77, 77]
    labels = np.full(m + 3, 7, np.int32)
    lp = labels.ctypes.data_as(C.POINTER(C.c_int32))
    ctx._check(lib.lv_map_planes(ctx.h, C.byref(p), None, lp, m + 3, None, 0, None))
    assert np.array_equal(labels[:m], ref["labels"]) and np.all(labels[m:] == 7)
    labels[:] = 7
    n.value = 123
    assert lib.lv_map_planes(ctx.h, C.byref(p), None, lp, m - 1, planes.ctypes.data_as(C.POINTER(capi.Plane)), 4, C.byref(n)) == LV_EINVAL   # capacity < m
    assert f"capacity {m - 1} < {m} living points" in lib.lv_last_error().decode()
    assert n.value == 123 and np.all(labels == 7) and int(planes["inliers"][2]) == 77


def test_the_entry_point_answers_the_rule_table(capi, room_ctx):
    """every case of tests/plane_cases.py through lv_map_planes itself: a refusal gives LV_EINVAL, its message, and writes nothing"""
    lib, ctx = capi.load_library(), room_ctx
    m = ctx.map_size()
    labels = np.full(m, 7, np.int32)
    n = C.c_size_t(123)
    refused = 0
    for c in pc.CASES:
        if c["rc"] == pc.LV_OK:
            continue
        p = None if c.get("null") else C.byref(capi.default_plane_params(**c["over"]))
        assert lib.lv_map_planes(ctx.h, p, None, labels.ctypes.data_as(C.POINTER(C.c_int32)), m, None, 0, C.byref(n)) == LV_EINVAL, c["name"]
        assert lib.lv_last_error().decode() == c["msg"], c["name"]
        refused += 1
    assert refused >= 30 and n.value == 123 and np.all(labels == 7)


# ---- a call while a background rebuild runs reads the active store and equals the one before
def test_during_a_background_rebuild(capi, room):
    xyz = room[0]
    kw = {**ROOM, "max_planes": 3}
    with capi.Context() as ctx:
        ctx.set_option("async_relinearise", 1)
        ctx.map_build(xyz)
        ctx.map_evict_box(np.array([-1e3, -1e3, -1e3], F), np.array([1e3, 1.0, 1e3], F), keep_inside=False)
        before = planes_of(capi, ctx, **kw)
        hold(before, pr.segment(ctx.map_fetch(), kw), "before the rebuild")
        ctx.set_option("async_relinearise_test_delay_ms", 400)
        ctx.map_relinearise_async()
        t0 = time.monotonic()
        while ctx.map_rebuild_status()["state"] in (4, 5) and time.monotonic() - t0 < 10:   # until the snapshot is taken
            ctx.map_size()
            time.sleep(0.001)
        assert ctx.map_rebuild_status()["state"] == 1
        during = planes_of(capi, ctx, **kw)
        assert ctx.map_rebuild_status()["state"] == 1                                        # (it did not wait for the rebuild)
        assert np.array_equal(during["labels"], before["labels"]) and during["planes"].tobytes() == before["planes"].tobytes()


# ---- planes.ground against cluster.ground_mask
def test_ground_helper_excludes_the_table_top(capi, room, room_ctx, tmp_path):
    from limo_velo_amd import cluster, planes

    xyz, kind = room
    mask, floor = planes.ground(room_ctx, **ROOM)
    ref = room_ref(room, max_planes=1, constraint=1, axis=(0.0, 0.0, 1.0), max_angle=float(np.deg2rad(10.0)))
    assert np.array_equal(mask, ref["labels"] == 0) and int(floor["inliers"]) == ref["planes"][0]["inliers"]
    assert mask[kind == 0].mean() > 0.99 and not mask[kind == 4].any() and floor["normal"][2] > 0.999
    by_normals = cluster.ground_mask(room_ctx.map_normals()["normals"], 15.0) == 0           # what the normals call ground
    assert by_normals[kind == 4].mean() > 0.8                                                  # ... includes the table top
    s = planes.signed_distance(floor, xyz)
    assert np.array_equal(np.abs(s) <= F(ROOM["distance"]), mask)
    w = planes.walls(room_ctx, max_planes=2, **ROOM)
    assert w["n_planes"] == 2 and {int(np.bincount(kind[w["labels"] == r]).argmax()) for r in range(2)} == {1, 2}
    out = planes.segment(room_ctx, **ROOM, max_planes=4)
    planes.save_ply(tmp_path / "room.ply", xyz, out["labels"])
    blob = (tmp_path / "room.ply").read_bytes()
    assert blob.startswith(b"ply\n") and len(blob) == blob.index(b"end_header\n") + 11 + 15 * len(xyz)
