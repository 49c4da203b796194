"""tests/occupancy_ref.py, the numpy statement of the occupancy grid's rule (include/limovelo_hip.h "Occupancy grid"), checked on its
own with exact integer / Fraction geometry before anything is held to it: every voxel a walk visits is met by the closed segment
qs-qe, consecutive voxels differ by one step on one axis, the walk has r_x + r_y + r_z steps and ends in ve; then the degenerate
walks, and the update and projection rules on small hand-made cases."""
from fractions import Fraction

import numpy as np

import occupancy_ref as ocr


def _paths(qs, qe):
    """Per ray the list of cells it stands in, ve included."""
    qe = np.asarray(qe, np.int64).reshape(-1, 3)
    steps, ve = ocr.walk(qs, qe)
    out = [[] for _ in range(len(qe))]
    for cells, alive in steps:
        for i in np.nonzero(alive)[0]:
            out[i].append(tuple(int(c) for c in cells[i]))
    for i in range(len(qe)):
        out[i].append(tuple(int(c) for c in ve[i]))
    return out


def _segment_meets_cell(qs, qe, cell):
    """The closed segment qs-qe (sub-units) meets the closed cube of the cell: slabs in exact arithmetic."""
    lo, hi = Fraction(0), Fraction(1)
    for a in range(3):
        d = int(qe[a]) - int(qs[a])
        c0, c1 = cell[a] * 256 - int(qs[a]), (cell[a] + 1) * 256 - int(qs[a])
        if d == 0:
            if not (c0 <= 0 <= c1):
                return False
            continue
        t0, t1 = Fraction(c0, d), Fraction(c1, d)
        lo, hi = max(lo, min(t0, t1)), min(hi, max(t0, t1))
    return lo <= hi


def _check(qs, qe):
    qs = np.broadcast_to(np.asarray(qs, np.int64), np.asarray(qe).reshape(-1, 3).shape)
    qe = np.asarray(qe, np.int64).reshape(-1, 3)
    for i, path in enumerate(_paths(qs, qe)):
        vs, ve = tuple(int(v) >> 8 for v in qs[i]), tuple(int(v) >> 8 for v in qe[i])
        assert path[0] == vs and path[-1] == ve
        assert len(path) - 1 == sum(abs(ve[a] - vs[a]) for a in range(3))
        for c0, c1 in zip(path, path[1:]):
            assert sorted(abs(c1[a] - c0[a]) for a in range(3)) == [0, 0, 1]
        for c in path:
            assert _segment_meets_cell(qs[i], qe[i], c), (qs[i], qe[i], c)
    return _paths(qs, qe)


def test_random_rays_follow_their_segment():
    rng = np.random.default_rng(3)
    qs = rng.integers(-300, 8 * 256 + 300, (300, 3))
    qe = rng.integers(-300, 8 * 256 + 300, (300, 3))
    _check(qs, qe)
    # one origin, many ends (the shape of a view), short rays included
    _check(np.array([1000, 1100, 900]), np.array([1000, 1100, 900]) + rng.integers(-700, 700, (200, 3)))


def test_axis_aligned_rays():
    for a in range(3):
        for sgn in (1, -1):
            qs = np.array([1030, 1040, 1050])
            qe = qs.copy()
            qe[a] += sgn * 900
            (path,) = _check(qs, qe[None])
            assert all(c[b] == path[0][b] for c in path for b in range(3) if b != a)
            assert len(path) == abs((int(qe[a]) >> 8) - (int(qs[a]) >> 8)) + 1


def test_exact_diagonals_break_ties_x_then_y_then_z():
    # from a cell's centre along (1, 1, 1): every boundary is a three-way tie
    (path,) = _check(np.array([128, 128, 128]), np.array([[128 + 512, 128 + 512, 128 + 512]]))
    assert path == [(0, 0, 0), (1, 0, 0), (1, 1, 0), (1, 1, 1), (2, 1, 1), (2, 2, 1), (2, 2, 2)]
    # the same backwards, and through lattice corners exactly
    (path,) = _check(np.array([640, 640, 640]), np.array([[128, 128, 128]]))
    assert path == [(2, 2, 2), (1, 2, 2), (1, 1, 2), (1, 1, 1), (0, 1, 1), (0, 0, 1), (0, 0, 0)]
    (path,) = _check(np.array([256, 256, 256]), np.array([[768, 768, 768]]))
    assert path == [(1, 1, 1), (2, 1, 1), (2, 2, 1), (2, 2, 2), (3, 2, 2), (3, 3, 2), (3, 3, 3)]
    # a two-way tie in y, z only
    (path,) = _check(np.array([10, 128, 128]), np.array([[20, 384, 384]]))
    assert path == [(0, 0, 0), (0, 1, 0), (0, 1, 1)]


def test_start_on_a_boundary_moving_down_and_no_move():
    # qs on the boundary x = 512 moving in -x: n = 0, the first step is taken at once
    (path,) = _check(np.array([512, 300, 300]), np.array([[200, 310, 300]]))
    assert path[:2] == [(2, 1, 1), (1, 1, 1)] and path[-1] == (0, 1, 1)
    (path,) = _check(np.array([512, 512, 512]), np.array([[511, 511, 511]]))
    assert path == [(2, 2, 2), (1, 2, 2), (1, 1, 2), (1, 1, 1)]
    (path,) = _check(np.array([700, 700, 700]), np.array([[700, 700, 700]]))
    assert path == [(2, 2, 2)]
    (path,) = _check(np.array([700, 700, 700]), np.array([[701, 699, 700]]))   # moves, but stays in its cell
    assert path == [(2, 2, 2)]
    (path,) = _check(np.array([-1, -256, -257]), np.array([[0, -256, -257]]))    # negative coordinates: arithmetic shift
    assert path == [(-1, -1, -2), (0, -1, -2)]


def test_quantisation_and_view_rules():
    prm = ocr.params(origin=(-1.0, -1.0, -1.0), resolution=0.5, nx=8, ny=8, nz=8)
    assert list(ocr.view_origin(prm, (0.0, 0.25, -1.0))) == [512, 640, 0]
    assert list(ocr.view_origin(prm, (-1.001, 0.0, 0.0)))[0] == -1
    assert ocr.view_origin(prm, (np.nan, 0.0, 0.0)) is None and ocr.view_origin(prm, (0.0, np.inf, 0.0)) is None
    assert ocr.view_origin(prm, (8192 * 0.5 - 1.0, 0.0, 0.0)) is None and ocr.view_origin(prm, (8191.5 * 0.5 - 1.0, 0.0, 0.0)) is not None
    Id = np.eye(3)
    pts = np.array([[2.0, 0, 0], [0.5, 0, 0], [np.nan, 0, 0], [0, np.inf, 0], [100.0, 0, 0], [0, 0, 80.0], [1.0, 0, 0]], np.float32)
    qe, hit = ocr.returns(prm, Id, (0.0, 0.0, 0.0), pts)
    # below min_range and non-finite are ignored; beyond max_range cut to max_range; exactly min_range / max_range kept as hits
    assert list(hit) == [True, False, True, True]
    assert [list(q) for q in qe] == [[1536, 512, 512], [41472, 512, 512], [512, 512, 41472], [1024, 512, 512]]


def test_update_and_projection_rules():
    prm = ocr.params(origin=(0.0, 0.0, 0.0), resolution=1.0, nx=8, ny=1, nz=1, min_range=0.1, max_range=6.0)
    # sensor in voxel 1, one return in voxel 5 and one in voxel 3: 3 is hit AND crossed, so hit only; 1, 2, 4 free; 5 hit
    view = (np.eye(3), (1.5, 0.5, 0.5), np.array([[4.0, 0, 0], [2.0, 0, 0]], np.float32))
    L, stats = ocr.integrate(prm, ocr.empty(prm), [view])
    want = np.full(8, np.nan, np.float32)
    want[[1, 2, 4]] = np.float32(-0.4)
    want[[3, 5]] = np.float32(0.85)
    assert ocr.same_bits(L.reshape(-1), want) and list(stats) == [2, 0, 3, 2]
    # clamping at both ends: 12 times the same view
    L, _ = ocr.integrate(prm, ocr.empty(prm), [view] * 12)
    assert L[0, 0, 5] == np.float32(3.5) and L[0, 0, 2] == np.float32(-2.0) and np.isnan(L[0, 0, 0])
    # a cut return frees its end voxel
    L, stats = ocr.integrate(prm, ocr.empty(prm), [(np.eye(3), (0.5, 0.5, 0.5), np.array([[30.0, 0, 0]], np.float32))])
    assert list(stats) == [1, 1, 7, 0] and np.all(L[0, 0, :7] == np.float32(-0.4)) and np.isnan(L[0, 0, 7])   # (cut at 6.0: ends in voxel 6)
    # projection: occupied beats free beats unknown, over the band only
    prm = ocr.params(nx=3, ny=1, nz=3)
    L = np.full((3, 1, 3), np.nan, np.float32)
    L[0, 0, 0], L[1, 0, 0] = 0.85, -0.4
    L[1, 0, 1] = -0.4
    L[2, 0, 2] = 0.4
    assert list(ocr.project(prm, L, 0, 2)[0]) == [100, 0, 100]
    assert list(ocr.project(prm, L, 1, 1)[0]) == [0, 0, -1]
    assert list(ocr.project(prm, L, -5, 0)[0]) == [100, -1, -1]
    assert list(ocr.project(prm, L, 3, 9)[0]) == [-1, -1, -1]
