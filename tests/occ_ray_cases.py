"""The grids, rays and views that tests/test_occ_ray_host.py (the host build of lv_ray.hpp) and tests/test_gpu_occ_ray.py (the kernels)
both hold to tests/occ_ray_ref.py, and the reference's answers for them, computed once per process."""
import functools

import numpy as np

import occ_ray_ref as orr
import occupancy_ref as ocr

F = np.float32
# the grid of tests/test_occupancy_host.py
PRM = ocr.params(origin=(-2.0, -1.5, -1.0), resolution=0.25, nx=19, ny=13, nz=9, min_range=0.3, max_range=4.0)
PLACES = ((0.1, 0.2, 0.3), (-3.3, 0.0, 0.1), (3.9, 2.7, 0.0), (0.0, 0.0, 2.1), (0.0, 0.0, -1.9), (2.749, 1.749, 1.249))
ID = np.eye(3, dtype=F)


def centre(prm, i, j, k):
    return (np.asarray(prm["origin"], np.float64) + (np.array([i, j, k]) + 0.5) * prm["resolution"]).astype(F)


def corner(prm, i, j, k):
    return (np.asarray(prm["origin"], np.float64) + np.array([i, j, k]) * prm["resolution"]).astype(F)


@functools.lru_cache(None)
def grid():
    """[9, 13, 19] f32 with all four states, L exactly l_occ and exactly l_free among them, and a corridor along x in row
    (j, k) = (6, 4): cells 2..10 free, cell 11 occupied, cell 1 unknown."""
    rng = np.random.default_rng(5)
    values = np.array([np.nan, PRM["l_free"], -2.0, -0.41, PRM["l_occ"], 0.85, 3.5, 0.0, 0.39, -0.39], F)
    prob = np.array([0.30, 0.15, 0.15, 0.12, 0.04, 0.03, 0.03, 0.06, 0.06, 0.06])
    L = values[rng.choice(len(values), size=(PRM["nz"], PRM["ny"], PRM["nx"]), p=prob)]
    L[4, 6, 2:11] = F(PRM["l_free"])
    L[4, 6, 11] = F(PRM["l_occ"])
    L[4, 6, 1] = np.nan
    L.setflags(write=False)
    st = orr.states(PRM, L)
    assert all((st == s).any() for s in (orr.FREE, orr.OCCUPIED, orr.UNKNOWN, orr.OTHER))
    assert (L == F(PRM["l_occ"])).any() and (L == F(PRM["l_free"])).any()
    return L


def _first(state):
    """(i, j, k) of the first voxel of grid() in that state."""
    k, j, i = np.argwhere(orr.states(PRM, grid()) == state)[0]
    return int(i), int(j), int(k)


@functools.lru_cache(None)
def rays():
    """{name: (from [n, 3], to [n, 3])} in world coordinates."""
    rng = np.random.default_rng(21)
    out = {}
    for p, t in enumerate(PLACES):   # inside; outside on each side: entering, missing and leaving at once
        d = rng.normal(size=(400, 3))
        d /= np.linalg.norm(d, axis=1)[:, None]
        frm = np.tile(np.array(t, F), (400, 1))
        out[f"random{p}"] = (frm, (frm + d * rng.uniform(0.1, 6.0, (400, 1))).astype(F))
    pts = np.array([centre(PRM, 8, 6, 4), centre(PRM, *_first(orr.OCCUPIED)), centre(PRM, *_first(orr.UNKNOWN)), (-3.0, 0.0, 0.0), (9.0, 9.0, 9.0)], F)
    out["from_is_to"] = (pts, pts.copy())
    # a stop in c_0 (occupied; unknown when stop_unknown), towards the grid's middle and out of the grid
    c0 = np.array([centre(PRM, *_first(orr.OCCUPIED)), centre(PRM, *_first(orr.UNKNOWN))] * 2, F)
    out["stop_in_c0"] = (c0, np.array([centre(PRM, 9, 6, 4)] * 2 + [(-5.0, -5.0, -5.0)] * 2, F))
    # a stop in ve: down the corridor into its occupied end, and up it into its unknown end
    out["stop_in_ve"] = (np.array([centre(PRM, 2, 6, 4), centre(PRM, 10, 6, 4)], F), np.array([centre(PRM, 11, 6, 4), centre(PRM, 1, 6, 4)], F))
    # ties: both ends on voxel corners, along the face and space diagonals in every sign combination
    dirs = [(sx, sy, sz) for sx in (-1, 0, 1) for sy in (-1, 0, 1) for sz in (-1, 0, 1) if abs(sx) + abs(sy) + abs(sz) >= 2]
    frm, to = [], []
    for base in ((8, 6, 4), (0, 0, 0), (19, 13, 9)):
        for d in dirs:
            for n in (1, 3, 7):
                frm.append(corner(PRM, *base))
                to.append(corner(PRM, *(np.array(base) + n * np.array(d))))
    out["ties"] = (np.array(frm, F), np.array(to, F))
    # negative cells: outside below the origin, moving away, along the grid, and into it
    out["negative"] = (np.array([(-3.0, -2.0, -1.5)] * 3 + [(-2.01, -1.51, -1.01)], F),
                       np.array([(-2.5, -3.0, -2.0), (-2.1, 1.0, -1.2), (1.0, 1.0, 1.0), (-1.9, -1.4, -0.9)], F))
    # ignored: NaN, inf, `from` 8192 voxels out, `to` quantising to 2^24; and one that is not
    o = np.array([0.1, 0.2, 0.3], F)
    bad = [((np.nan, 0, 0), o), (o, (0, np.nan, 0)), ((0, 0, np.inf), o), (o, (-np.inf, 0, 0)), ((-2.0 + 8192 * 0.25, 0, 0), o),
           ((0, -1.5 - 8192 * 0.25, 0), o), (o, (-2.0 + 65536 * 0.25, 0, 0)), (o, (0, 0, -1.0 - 65537 * 0.25)), (o, (1.0, 1.0, 1.0))]
    out["ignored"] = (np.array([b[0] for b in bad], F), np.array([b[1] for b in bad], F))
    return out


@functools.lru_cache(None)
def ray_answers():
    """{(name, stop_unknown): the reference's results}"""
    return {(name, su): orr.raycast(PRM, grid(), frm, to, su) for name, (frm, to) in rays().items() for su in (False, True)}


@functools.lru_cache(None)
def plain_grid():
    """Free everywhere but for an unknown voxel (12, 6, 4) and an occupied one (12, 8, 4)."""
    L = np.full((PRM["nz"], PRM["ny"], PRM["nx"]), -1.0, F)
    L[4, 6, 12] = np.nan
    L[4, 8, 12] = 2.0
    L.setflags(write=False)
    return L


def _rot(rng):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]], F)


@functools.lru_cache(None)
def gain_views():
    """{name: (grid, [(R, t, points)])}"""
    t = centre(PRM, 8, 6, 4)
    out = {}
    # two rays along one row through the unknown voxel (12, 6, 4)
    out["twice"] = (plain_grid(), [(ID, t, np.array([(1.5, 0.0, 0.0), (1.5, 0.05, 0.0)], F))])
    # one ray stopped by the occupied voxel (12, 8, 4), one passing beside it
    out["stopped"] = (plain_grid(), [(ID, t, np.array([(1.5, 0.75, 0.0), (1.5, 0.0, 0.25)], F))])
    # one return cut at max_range = 4 (it leaves the grid), one below min_range = 0.3 (ignored), one plain
    out["ranges"] = (plain_grid(), [(ID, t, np.array([(9.0, 0.0, 0.0), (0.2, 0.0, 0.0), (0.0, 0.5, 0.0)], F))])
    # no evidence: no returns, a non-finite origin, an origin too far; then one that has some
    pts = np.array([(1.0, 0.0, 0.0), (0.0, 1.0, 0.0)], F)
    out["no_evidence"] = (grid(), [(ID, t, np.zeros((0, 3), F)), (ID, np.array([np.nan, 0, 0], F), pts), (ID, np.array([9000.0, 0, 0], F), pts),
                                   (ID, t, pts)])
    rng = np.random.default_rng(33)
    views = []
    for place in PLACES:
        d = rng.normal(size=(400, 3))
        d /= np.linalg.norm(d, axis=1)[:, None]
        views.append((_rot(rng), np.array(place, F), (d * rng.uniform(0.1, 6.0, (400, 1))).astype(F)))
    out["random"] = (grid(), views)
    return out


@functools.lru_cache(None)
def gain_answers():
    return {name: orr.view_gain(PRM, L, views) for name, (L, views) in gain_views().items()}
