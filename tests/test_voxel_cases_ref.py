"""CPU tests of what tests/test_gpu_voxel_grid.py compares the device with: the cases of tests/voxel_cases.py can tell a
voxel grid that keeps pcl::VoxelGrid's summation order from one that does not.

* the numpy statement of the rule (f32 floor by x * (1/leaf), mixed-radix leaf order, stable sort, explicit sequential f32
  sum) equals oracle.voxelgrid bit for bit on every case;
* every centroid lies within m * 2**-24 * max|x| per axis of the f64 mean of its leaf (a sequential f32 sum of m values errs
  by at most (m-1) u sum|x|, the divide adds one rounding; u = 2**-24);
* the inputs are sensitive to the order of the sum: summing a leaf in reverse, or pairwise, changes bits;
* the structure each case is named after (populations, head parities, straddled positions, points in and out) holds in the
  reference's own sorted order."""
import numpy as np
import pytest

import voxel_cases as vc

CASES = vc.cases()
IDS = [c.name for c in CASES]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _by_name(name):
    return next(c for c in CASES if c.name == name)


def _leaves(case):
    """(first sorted position, population) of every leaf, from the reference's sorted order of the kept points."""
    _, heads, counts = vc.leaf_order(vc.kept(case), case.leaf)
    return heads, counts


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_identity_deskew_leaves_the_points_as_built(oracle, case):
    """What the oracle's voxel grid is given (behind its ingest and de-skew) is the case's kept points, in input order: the
    populations hold where the voxel grid runs."""
    assert np.array_equal(vc.voxel_input(case), vc.kept(case))
    if case.drop is not None:
        assert case.drop.any() and len(case.drop) == len(case.xyz)
        if case.entry == "downsample":
            assert np.array_equal(~np.isfinite(case.xyz).all(axis=1), case.drop)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_numpy_rule_equals_the_oracle(oracle, case):
    pts = vc.kept(case)
    want = vc.expected(case)
    if len(pts) == 0:
        assert len(want) == 0
        return
    got = vc.reference(pts, case.leaf)
    assert got.shape == want.shape and np.array_equal(_bits(got), _bits(want))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_centroids_lie_within_the_forward_error_bound(case):
    pts = vc.kept(case)
    if len(pts) == 0:
        return
    order, heads, counts = vc.leaf_order(pts, case.leaf)
    s = pts[order].astype(np.float64)
    cen = vc.reference(pts, case.leaf).astype(np.float64)
    mean = np.add.reduceat(s, heads, axis=0) / counts[:, None]
    amax = np.maximum.reduceat(np.abs(s), heads, axis=0)
    bound = counts[:, None] * 2.0 ** -24 * amax
    assert (np.abs(cen - mean) <= bound).all(), float((np.abs(cen - mean) / np.maximum(bound, 1e-300)).max())


@pytest.mark.parametrize("case", [c for c in CASES if len(vc.kept(c)) and "faces" not in c.name and "/" not in c.name],
                         ids=lambda c: c.name)
def test_the_order_of_the_sum_shows_in_the_bits(case):
    """Multi-leaf cases: at least a quarter of the leaves with >= 8 members change a bit when summed in reverse, and when
    summed pairwise — and when every whole chunk of eight members is summed backwards, the slip a read-ahead loop invites.
    One leaf with >= 8 members: every alternative changes a bit."""
    rev, pair, chunks = vc.order_sensitive(vc.kept(case), case.leaf)
    if case.one_leaf:
        if len(vc.kept(case)) >= 8:
            assert rev.all() and pair.all() and chunks.all()
        return
    if len(rev) == 0:
        pytest.fail("a multi-leaf case without a leaf of 8 or more members")
    print(f"{case.name}: changed by reverse {rev.mean():.2f}, pairwise {pair.mean():.2f}, chunks of 8 backwards {chunks.mean():.2f}")
    assert rev.mean() >= 0.25 and pair.mean() >= 0.25 and chunks.mean() >= 0.25, (rev.mean(), pair.mean(), chunks.mean())


@pytest.mark.parametrize("case", [c for c in CASES if "faces" not in c.name and len(vc.kept(c))], ids=lambda c: c.name)
def test_leaves_are_built_as_stated(case):
    pts = vc.kept(case)
    order, heads, counts = vc.leaf_order(pts, case.leaf)
    allowed = set(vc.POPULATIONS) | ({case.big} if case.big else set())
    if case.one_leaf:
        assert len(counts) == 1 and counts[0] == len(pts)
        return
    far = np.abs(pts).max(axis=1) > 1e4                    # the point that makes a route decline: alone in its leaf
    assert set(counts.tolist()) <= allowed, set(counts.tolist()) - allowed
    assert np.linalg.norm(pts.astype(np.float64), axis=1).min() >= 30.0
    assert (pts[~far] < 0).any() and (pts[~far] > 0).any()          # leaves with negative coordinates beside positive ones
    if len(counts) >= 12:
        assert all((pts[~far, a] < 0).any() and (pts[~far, a] > 0).any() for a in range(3))
    # no two members of a leaf are neighbours in the input
    leaf_of = np.empty(len(pts), np.int64)
    leaf_of[order] = np.repeat(np.arange(len(counts)), counts)
    assert (leaf_of[1:] != leaf_of[:-1]).all()
    # full mantissas: the low bits of the members are not all zero
    low = _bits(pts[~far]) & 0xFF
    assert len(np.unique(low)) >= min(200, len(pts) // 2)


def _straddles(heads, counts, pos):
    """A leaf with members on both sides of the edge pos-1 | pos."""
    return bool(((heads < pos) & (heads + counts > pos)).any())


def test_small_route_structure():
    for name in ("small-mix-2048", "small-mix-2048-window"):
        c = _by_name(name)
        heads, counts = _leaves(c)
        assert len(c.xyz) == vc.SMALL_WINDOW and c.route == vc.SMALL
        assert set(counts.tolist()) == set(vc.POPULATIONS)
        assert (heads % 2 == 0).sum() >= 4 and (heads % 2 == 1).sum() >= 4
        # heads of leaves with >= 8 members on both parities: the two elements of a thread both start long walks
        assert {int(h) % 2 for h, m in zip(heads, counts) if m >= 8} == {0, 1}
        assert _straddles(heads, counts, 128) and _straddles(heads, counts, 1024)
    c = _by_name("small-short-mix-leaf0.2")
    heads, counts = _leaves(c)
    assert c.leaf == np.float32(0.2) or c.leaf == 0.2
    assert set(counts.tolist()) == set(vc.POPULATIONS) and {int(h) % 2 for h in heads} == {0, 1}
    assert sorted(len(c.xyz) for c in CASES if c.one_leaf and c.route == vc.SMALL) == [1, 2, 7, 8, 9, 64, 65, 2047, 2048]
    for m in (7, 8, 9, 16, 17):
        for pre in ("small", "general"):
            c = _by_name(f"{pre}-last-run-{m}")
            heads, counts = _leaves(c)
            assert counts[-1] == m and heads[-1] + m == len(c.xyz)
            assert (len(c.xyz) <= vc.SMALL_WINDOW) == (pre == "small")
    for c in CASES:   # every small input also runs on the general route
        if c.route == vc.SMALL:
            assert len(c.xyz) <= vc.SMALL_WINDOW
            t = _by_name(c.name + "/general")
            assert t.xyz is c.xyz and t.route == vc.GENERAL and dict(t.options) == {"small_window": 0, "large_window": 0}
            if c.entry == "window":   # ... and, from the LiDAR buffer, on the large route
                t = _by_name(c.name + "/large")
                assert t.xyz is c.xyz and t.route == vc.LARGE and dict(t.options) == {"small_window": 0}


def test_large_route_structure():
    for c in CASES:
        if c.route == vc.LARGE:
            assert c.entry == "window" and len(c.xyz) <= vc.WT_IN and len(vc.expected(c)) <= vc.WT_OUT
            # beyond the small route's limit, or a small window with small_window off ("/large")
            assert (len(c.xyz) > vc.SMALL_WINDOW) != (dict(c.options) == {"small_window": 0})
    c = _by_name("large-one-leaf-7000")
    assert len(c.xyz) == 7000 > vc.WT_STAGE
    c = _by_name("large-leaf-straddles-6144")
    heads, counts = _leaves(c)
    assert len(c.xyz) > vc.WT_STAGE and _straddles(heads, counts, vc.WT_STAGE)
    assert set(counts.tolist()) == set(vc.POPULATIONS)
    c = _by_name("large-leaf-spans-a-stage")
    heads, counts = _leaves(c)
    big = np.argmax(counts)
    assert len(c.xyz) > 2 * vc.WT_STAGE and counts[big] >= 6200
    assert heads[big] < vc.WT_STAGE and heads[big] + counts[big] > 2 * vc.WT_STAGE      # straddles 6144 AND 12288
    assert (heads > 2 * vc.WT_STAGE).any()                                              # leaves wholly inside the third stage
    for name, n_out, route in (("large-1024-out", 1024, vc.LARGE), ("large-1025-out", 1025, vc.LARGE), ("large-4096-out", 4096, vc.LARGE),
                               ("large-4097-out-declines", 4097, vc.GENERAL)):
        c = _by_name(name)
        assert len(vc.expected(c)) == n_out and c.route == route and vc.SMALL_WINDOW < len(c.xyz) <= vc.WT_IN
    c = _by_name("large-16384-in")
    assert len(c.xyz) == vc.WT_IN and c.route == vc.LARGE
    c = _by_name("general-16385-in")
    assert len(c.xyz) == vc.WT_IN + 1 and c.route == vc.GENERAL and c.entry == "window"
    c = _by_name("large-dropped-behind-the-last-leaf")
    assert c.drop[0] and c.drop[len(c.xyz) // 2] and c.drop[-41:].all() and not c.drop[-42] and c.drop.sum() == 43
    heads, counts = _leaves(c)
    assert counts[-1] >= 2                     # the last leaf's end is a count that shows in its centroid
    c = _by_name("large-all-dropped")
    assert c.drop.all() and len(vc.expected(c)) == 0 and c.route == vc.LARGE


def test_decline_and_general_structure():
    c = _by_name("small-declines-8e15-cells")
    inv = np.float32(1.0) / np.float32(c.leaf)
    ext = np.floor(c.xyz.max(axis=0) * inv).astype(np.int64) - np.floor(c.xyz.min(axis=0) * inv).astype(np.int64) + 1
    cells = float(ext[0]) * float(ext[1]) * float(ext[2])
    assert len(c.xyz) <= vc.SMALL_WINDOW and c.route == vc.GENERAL and 4.0e15 <= cells < 2.0 ** 62
    c = _by_name("large-declines-6e5-m")
    assert vc.SMALL_WINDOW < len(c.xyz) <= vc.WT_IN and c.route == vc.GENERAL and c.entry == "window"
    assert np.floor(np.abs(c.xyz).max() * np.float32(2.0)) > 2 ** 20 and len(vc.expected(c)) <= vc.WT_OUT
    assert len(_by_name("general-16400-downsample").xyz) == 16400
    for entry in ("downsample", "deskew", "window"):
        c = _by_name(f"small-dropped-{entry}")
        n = len(c.xyz)
        assert c.drop[0] and c.drop[n // 2] and c.drop[-1] and c.entry == entry
        c = _by_name(f"small-all-dropped-{entry}")
        assert c.drop.all() and len(vc.expected(c)) == 0
    c = _by_name("general-dropped-deskew")
    assert c.drop[0] and c.drop[len(c.xyz) // 2] and c.drop[-1] and len(c.xyz) > vc.SMALL_WINDOW
    assert max(len(c.xyz) for c in CASES) <= 16400


@pytest.mark.parametrize("leaf", [0.5, 0.2])
def test_face_cases_sit_on_the_faces(leaf):
    c = _by_name(f"small-faces-leaf{leaf}")
    lf = np.float32(leaf)
    v = np.unique(_bits(c.xyz))
    for k in (-3, -1, 1, 3):
        assert _bits(np.float32(k) * lf) in v
    assert 0x80000000 in v and 0 in v                       # -0.0 beside +0.0
    _, heads, counts = vc.leaf_order(c.xyz, leaf)
    assert counts.max() >= 8 and counts.min() >= 1
    # -0.0 and +0.0 share a leaf; a face belongs to the leaf above it
    inv = np.float32(1.0) / lf
    assert np.floor(np.float32(-0.0) * inv) == np.floor(np.float32(0.0) * inv) == 0
    assert np.floor(lf * inv) == 1 and np.floor(np.nextafter(lf, np.float32(0)) * inv) == 0
