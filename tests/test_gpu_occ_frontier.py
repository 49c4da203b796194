"""GPU tests of the frontiers (lv_frontier.hip; include/limovelo_hip.h "Frontiers") against the statement of the rule in
tests/frontier_ref.py.  The rule is integer arithmetic once the states are decided, so everything is held to equality: labels,
cluster records, stats, best_p and best_cell.  The grids are set with occ_load.
The kernels label in tiles of 32 x 32 cells (planar) and 32 x 8 x 4 cells (3-D): the grids below have no dimension that is a multiple
of its tile edge, and x spans at least three tiles."""
import ctypes as C
import functools

import numpy as np
import pytest

import frontier_ref as fr
import occupancy_ref as ocr

pytestmark = pytest.mark.gpu

LV_OK, LV_EINVAL, LV_ESTATE = 0, -1, -4
F = np.float32
TILE = {1: (32, 32, 1), 0: (32, 8, 4)}   # by planar: the tile edges (x, y, z) of lv_frontier.hip
TABLE = np.array([200, 90, 50], np.uint8)


@pytest.fixture(scope="module")
def capi(lv):
    from limo_velo_amd import capi as c

    return c


def _prm(nx, ny, nz):
    return ocr.params(origin=(-1.0, 0.5, 2.0), resolution=0.25, nx=nx, ny=ny, nz=nz)


def _centre(prm, i, j, k=0):
    return (np.array(prm["origin"]) + (np.array([i, j, k]) + 0.5) * prm["resolution"]).astype(F)


def _context(capi, prm, L):
    ctx = capi.Context()
    ctx.occ_configure(capi.default_occupancy_params(**prm))
    ctx.occ_load(L)
    return ctx


def _hold(capi, ctx, prm, L, fp, ref=None):
    """The GPU's frontier of the grid last loaded equals frontier_ref's.  Returns the reference (labels, clusters, stats)."""
    rl, rcl, rst = ref if ref is not None else fr.build(prm, L, fp)
    st = ctx.occ_frontier_build(capi.default_frontier_params(**fp))
    labels, cl = ctx.occ_frontier_fetch(), ctx.occ_frontier_clusters()
    assert labels.shape == rl.shape and np.array_equal(labels, rl), (fp, f"{np.sum(labels != rl)} labels differ")
    assert list(st) == list(rst), (fp, st, rst)
    assert cl.dtype == fr.CLUSTER_DTYPE and np.array_equal(cl, rcl), fp
    i = ctx.occ_frontier_info()
    assert (i.built, i.stale, i.n_clusters, i.planar, i.nz) == (1, 0, len(rcl), int(fp["planar"] != 0), 1 if fp["planar"] else prm["nz"])
    assert (i.nx, i.ny) == (prm["nx"], prm["ny"]) and [getattr(i.params, f) for f in fr.FIELDS] == [fp[f] for f in fr.FIELDS]
    return rl, rcl, rst


def _crosses_a_seam(cl, planar):
    t = np.array(TILE[planar])
    return bool(np.any(cl["lo"] // t != cl["hi"] // t))


@functools.lru_cache(maxsize=None)
def _random_case(planar):
    nx, ny, nz = (150, 70, 5) if planar else (70, 45, 19)
    prm = _prm(nx, ny, nz)
    return prm, fr.random_logodds(np.random.default_rng(11 + planar), (nz, ny, nx), prm, 0.55 if planar else 0.05)


# ---- 1. random grids
@pytest.mark.parametrize("conn", [6, 18, 26])
def test_random_grid_3d(capi, conn):
    prm, L = _random_case(0)
    fp = fr.fparams(connectivity=conn)
    ref = fr.build(prm, L, fp)
    assert len(ref[1]) > 100 and _crosses_a_seam(ref[1], 0)   # (the case cannot pass trivially)
    with _context(capi, prm, L) as ctx:
        _hold(capi, ctx, prm, L, fp, ref)
        _hold(capi, ctx, prm, L, fr.fparams(connectivity=conn, min_size=4))


@pytest.mark.parametrize("conn", [4, 8])
def test_random_grid_planar_band(capi, conn):
    prm, L = _random_case(1)
    fp = fr.fparams(planar=1, k_lo=1, k_hi=3, connectivity=conn)
    ref = fr.build(prm, L, fp)
    assert len(ref[1]) > 100 and _crosses_a_seam(ref[1], 1)
    with _context(capi, prm, L) as ctx:
        _hold(capi, ctx, prm, L, fp, ref)
        for k_lo, k_hi in ((0, 4), (-3, 0), (4, 99), (7, 9)):   # all layers; clipped below; clipped above; clipped to nothing
            _hold(capi, ctx, prm, L, fr.fparams(planar=1, k_lo=k_lo, k_hi=k_hi, connectivity=conn, min_size=2))


# ---- 2. a serpentine through every tile: one component by a chain of seam joins
@pytest.mark.parametrize("dims,planar,conn", [((70, 70, 1), 1, 4), ((70, 70, 2), 1, 8), ((67, 19, 3), 0, 6), ((67, 19, 3), 0, 26)])
def test_serpentine(capi, dims, planar, conn):
    nx, ny, nz = dims
    prm = _prm(nx, ny, nz)
    L = fr.serpentine(prm, nx, ny, nz)
    fp = fr.fparams(planar=planar, k_lo=0, k_hi=nz - 1, connectivity=conn)
    ref = fr.build(prm, L, fp)
    t = TILE[planar]
    assert len(ref[1]) == 1 and list(ref[1][0]["hi"] // t) == [(nx - 1) // t[0], (ny - 1) // t[1], 0] and list(ref[1][0]["lo"] // t) == [0, 0, 0]
    with _context(capi, prm, L) as ctx:
        _hold(capi, ctx, prm, L, fp, ref)


# ---- 3. size ties are numbered by `first`; min_size drops the smaller of two
def test_size_ties_and_min_size(capi):
    prm = _prm(70, 37, 1)
    L = np.full((1, 37, 70), np.nan, F)
    L[0, 30, 60:66] = prm["l_min"]   # 6 cells, first = 30 * 70 + 60
    L[0, 3, 29:35] = prm["l_min"]    # 6 cells across the seam at x = 32, first = 3 * 70 + 29: the tie goes to it
    L[0, 20, 5:9] = prm["l_min"]     # 4 cells
    with _context(capi, prm, L) as ctx:
        for fp in (fr.fparams(planar=1, connectivity=4), fr.fparams(connectivity=6)):
            _, cl, _ = _hold(capi, ctx, prm, L, fp)
            assert list(cl["size"]) == [6, 6, 4] and list(cl["first"]) == [3 * 70 + 29, 30 * 70 + 60, 20 * 70 + 5]
            labels, cl, st = _hold(capi, ctx, prm, L, dict(fp, min_size=5))
            assert list(cl["size"]) == [6, 6] and labels.reshape(37, 70)[20, 6] == -1 and list(st) == [16, 70 * 37 - 16, 16, 2]


# ---- 4. no frontier at all
@pytest.mark.parametrize("what", ["unknown", "free", "occupied"])
def test_no_frontier(capi, what):
    prm = _prm(35, 9, 5)
    L = np.full((5, 9, 35), dict(unknown=np.nan, free=prm["l_min"], occupied=prm["l_max"])[what], F)
    with _context(capi, prm, L) as ctx:
        for fp in (fr.fparams(connectivity=18), fr.fparams(planar=1, k_lo=0, k_hi=4, connectivity=8)):
            labels, cl, st = _hold(capi, ctx, prm, L, fp)
            assert len(cl) == 0 and np.all(labels == -1) and st[2] == st[3] == 0
            n = C.c_size_t(9)
            assert ctx.lib.lv_occ_frontier_clusters(ctx.h, None, 0, C.byref(n)) == LV_OK and n.value == 0
            n = C.c_size_t(9)
            one = np.zeros(1, capi.FRONTIER_CLUSTER_DTYPE)
            assert ctx.lib.lv_occ_frontier_clusters(ctx.h, one.ctypes.data_as(C.POINTER(capi.FrontierCluster)), 0, C.byref(n)) == LV_OK and n.value == 0
            ctx.occ_distance_build(capi.default_distance_params(planar=fp["planar"], k_lo=0, k_hi=4))
            ctx.occ_plan_build(_centre(prm, 1, 1, 1)[None], TABLE, capi.default_plan_params(connectivity=8 if fp["planar"] else 26))
            bp, bc = (C.c_uint32 * 1)(3), (C.c_int32 * 1)(4)
            assert ctx.lib.lv_occ_frontier_rank(ctx.h, 2, bp, bc, 0) == LV_OK and bp[0] == 3 and bc[0] == 4


# ---- 5. degenerate grids
@pytest.mark.parametrize("dims", [(1, 1, 1), (1, 37, 1), (33, 1, 9)])
def test_degenerate_grids(capi, dims):
    nx, ny, nz = dims
    prm = _prm(nx, ny, nz)
    rng = np.random.default_rng(nx + ny + nz)
    with _context(capi, prm, fr.random_logodds(rng, (nz, ny, nx), prm)) as ctx:
        for p_unknown in (0.0, 0.3, 0.6, 1.0):
            L = fr.random_logodds(rng, (nz, ny, nx), prm, p_unknown)
            ctx.occ_load(L)
            for fp in (fr.fparams(connectivity=6), fr.fparams(connectivity=26), fr.fparams(planar=1, k_lo=0, k_hi=nz - 1, connectivity=4),
                       fr.fparams(planar=1, k_lo=0, k_hi=0, connectivity=8)):
                _hold(capi, ctx, prm, L, fp)


# ---- 6. the result is a snapshot
def test_snapshot(capi):
    prm = _prm(40, 21, 6)
    rng = np.random.default_rng(5)
    L = fr.random_logodds(rng, (6, 21, 40), prm)
    with _context(capi, prm, L) as ctx:
        lib = ctx.lib
        info = capi.FrontierInfo()
        assert ctx.occ_frontier_info().built == 0
        lab = np.zeros(40 * 21 * 6, np.int32)
        n = C.c_size_t(7)
        for rc in (lib.lv_occ_frontier_fetch(ctx.h, lab.ctypes.data_as(C.POINTER(C.c_int32)), lab.size), lib.lv_occ_frontier_clusters(ctx.h, None, 0, C.byref(n)),
                   lib.lv_occ_frontier_rank(ctx.h, 0, (C.c_uint32 * 1)(), None, 1)):
            assert rc == LV_ESTATE   # before a build
        assert n.value == 7
        ctx.occ_distance_build(capi.default_distance_params())
        ctx.occ_plan_build(_centre(prm, 3, 3, 3)[None], TABLE, capi.default_plan_params(connectivity=26))
        grid0, s20, (P0, c0) = ctx.occ_fetch(), ctx.occ_distance_fetch()[0], ctx.occ_plan_fetch()
        fp = fr.fparams(connectivity=18)
        rl, rcl, _ = _hold(capi, ctx, prm, L, fp)
        # building changed no bit of the grid, the distance field or the plan
        assert ocr.same_bits(ctx.occ_fetch(), grid0) and np.array_equal(ctx.occ_distance_fetch()[0], s20)
        P1, c1 = ctx.occ_plan_fetch()
        assert np.array_equal(P1, P0) and np.array_equal(c1, c0) and ctx.occ_plan_info().stale == 0 and ctx.occ_distance_info().stale == 0
        # fetch and clusters judge their capacity
        assert lib.lv_occ_frontier_fetch(ctx.h, lab.ctypes.data_as(C.POINTER(C.c_int32)), lab.size - 1) == LV_EINVAL
        out = np.zeros(len(rcl), capi.FRONTIER_CLUSTER_DTYPE)
        n = C.c_size_t(0)
        assert lib.lv_occ_frontier_clusters(ctx.h, out.ctypes.data_as(C.POINTER(capi.FrontierCluster)), len(rcl) - 1, C.byref(n)) == LV_EINVAL
        assert n.value == len(rcl) and not out.view(np.uint8).any()
        bp = np.full(len(rcl), 7, np.uint32)
        assert lib.lv_occ_frontier_rank(ctx.h, 1, bp.ctypes.data_as(C.POINTER(C.c_uint32)), None, len(rcl) - 1) == LV_EINVAL and np.all(bp == 7)
        # a refused build leaves the old result
        bad = capi.default_frontier_params(connectivity=8)
        assert lib.lv_occ_frontier_build(ctx.h, C.byref(bad), None) == LV_EINVAL
        assert ctx.occ_frontier_info().built == 1 and np.array_equal(ctx.occ_frontier_fetch(), rl)
        # a new grid: stale, the old labels are still fetched
        L2 = fr.random_logodds(rng, (6, 21, 40), prm)
        ctx.occ_load(L2)
        i = ctx.occ_frontier_info()
        assert (i.built, i.stale) == (1, 1) and np.array_equal(ctx.occ_frontier_fetch(), rl) and np.array_equal(ctx.occ_frontier_clusters(), rcl)
        _hold(capi, ctx, prm, L2, fp)   # a new build replaces it: stale = 0
        ctx.occ_clear()
        assert ctx.occ_frontier_info().stale == 1
        ctx.occ_frontier_clear()
        assert ctx.occ_frontier_info().built == 0
        _hold(capi, ctx, prm, np.full((6, 21, 40), np.nan, F), fp)
        ctx.occ_configure(capi.default_occupancy_params(**prm))
        assert lib.lv_occ_frontier_info(ctx.h, C.byref(info)) == LV_OK and info.built == 0 and info.nx == 0


# ---- 7. rank
def _hold_rank(ctx, rl, rcl, reaches=(0, 2, 8)):
    P, _ = ctx.occ_plan_fetch()
    for reach in reaches:
        bp, bc = ctx.occ_frontier_rank(reach)
        rp, rc = fr.rank(rl, len(rcl), P, reach)
        assert np.array_equal(bp, rp) and np.array_equal(bc, rc), reach
    return P


def test_rank_serpentine(capi):
    nx, ny, nz = 70, 41, 1
    prm = _prm(nx, ny, nz)
    L = fr.serpentine(prm, nx, ny, nz)
    with _context(capi, prm, L) as ctx:
        fp = fr.fparams(planar=1, connectivity=4)
        rl, rcl, _ = _hold(capi, ctx, prm, L, fp)
        ctx.occ_distance_build(capi.default_distance_params(planar=1, unknown_is_obstacle=1))
        ctx.occ_plan_build(_centre(prm, 1, 1)[None], TABLE, capi.default_plan_params(connectivity=4))
        P = _hold_rank(ctx, rl, rcl)
        bp, bc = ctx.occ_frontier_rank(0)
        assert bp[0] == 0 and bc[0] == nx + 1 and np.sum(P != fr.UNREACHED) == rcl[0]["size"]   # (the goal cell is a member)
        # a plan with no usable goal: nothing is reached
        ctx.occ_plan_build(_centre(prm, 0, 0)[None], TABLE, capi.default_plan_params(connectivity=4))
        bp, bc = ctx.occ_frontier_rank(8)
        assert list(bp) == [fr.UNREACHED] and list(bc) == [-1]
        _hold_rank(ctx, rl, rcl)
        # a plan of other cells: refused
        ctx.occ_distance_build(capi.default_distance_params())
        ctx.occ_plan_build(_centre(prm, 1, 1)[None], TABLE, capi.default_plan_params(connectivity=6))
        one = (C.c_uint32 * 1)(5)
        assert ctx.lib.lv_occ_frontier_rank(ctx.h, 0, one, None, 1) == LV_ESTATE and one[0] == 5
        ctx.occ_plan_clear()
        assert ctx.lib.lv_occ_frontier_rank(ctx.h, 0, one, None, 1) == LV_ESTATE


@pytest.mark.parametrize("planar", [1, 0])
def test_rank_random(capi, planar):
    nx, ny, nz = (150, 70, 5) if planar else (70, 21, 9)
    prm = _prm(nx, ny, nz)
    rng = np.random.default_rng(3 + planar)
    L = fr.random_logodds(rng, (nz, ny, nx), prm, 0.2)
    fp = fr.fparams(planar=1, k_lo=0, k_hi=0, connectivity=8) if planar else fr.fparams(connectivity=26)
    with _context(capi, prm, L) as ctx:
        rl, rcl, _ = _hold(capi, ctx, prm, L, fp)
        ctx.occ_distance_build(capi.default_distance_params(planar=planar, k_lo=0, k_hi=0))
        k, j, i = np.argwhere((rl[None] if planar else rl) >= 0)[len(rcl) // 2]
        st = ctx.occ_plan_build(_centre(prm, i, j, k)[None], TABLE, capi.default_plan_params(connectivity=8 if planar else 26))
        assert st[0] == 1   # (the goal is a frontier cell: free, so no obstacle)
        _hold_rank(ctx, rl, rcl, (0, 2, 8) if planar else (0, 2))
        # stale results are ranked as they are
        ctx.occ_load(L)
        assert ctx.occ_frontier_info().stale == 1
        _hold_rank(ctx, rl, rcl, (2,))


# ---- 8. occupancy.frontiers / occupancy.explore on two rooms
def test_explore_two_rooms(capi):
    from limo_velo_amd import occupancy

    prm = ocr.params(origin=(0.0, 0.0, 0.0), resolution=0.25, nx=40, ny=16, nz=1)
    L = np.full((1, 16, 40), prm["l_max"], F)     # walls everywhere ...
    L[0, 1:15, 1:19] = prm["l_min"]               # ... but room A,
    L[0, 1:15, 21:39] = prm["l_min"]              # room B
    L[0, 7:9, 19:21] = prm["l_min"]               # and the door between them
    L[0, 15, 5:8] = np.nan                        # a hole in A's outer wall
    L[0, 0, 30:33] = np.nan                       # and one in B's
    robot = np.array([10.5 * 0.25, 7.5 * 0.25, 0.1], F)
    with _context(capi, prm, L) as ctx:
        labels, cl = occupancy.frontiers(ctx, z_band=(0.0, 0.25), connectivity=4)
        rl, rcl, _ = fr.build(prm, L, fr.fparams(planar=1, connectivity=4))
        assert np.array_equal(labels, rl) and list(cl["first"]) == [1 * 40 + 30, 14 * 40 + 5] and list(cl["size"]) == [3, 3]
        assert np.allclose(cl["rep_xyz"][1], [6.5 * 0.25, 14.5 * 0.25, 0.0]) and np.allclose(cl["centre_xyz"][0], [31.5 * 0.25, 1.5 * 0.25, 0.0])
        found, lines = occupancy.explore(ctx, robot, 0.1, z_band=(0.0, 0.25))
        assert len(found) == 2 and list(found["label"]) == [1, 0] and found["best_p"][0] < found["best_p"][1] < capi.LV_PLAN_UNREACHED
        assert found["target_xyz"][0][0] < 19 * 0.25 < found["target_xyz"][1][0]   # the first target lies in room A, the second in B
        for c in range(2):
            assert np.allclose(lines[c][0], robot[:2]) and np.allclose(lines[c][-1], found["target_xyz"][c][:2])
        assert len(lines[0]) < len(lines[1])
