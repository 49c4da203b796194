"""GPU tests of the planner (lv_plan.hip; include/limovelo_hip.h "Planner") against the statement of the rule in tests/plan_ref.py.
Edge costs are integers and the potential is the unique fixpoint of relaxation, so everything is held to equality on every cell and
every path: cost bytes, P, stats, status, path costs, offsets and path cells.  The grids are set with occ_load, then
occ_distance_build, then the plan; the distance field the reference plans on is distance_ref's."""
import ctypes as C

import numpy as np
import pytest

import distance_ref as dr
import occupancy_ref as ocr
import plan_ref as pr

pytestmark = pytest.mark.gpu

LV_EINVAL, LV_ESTATE = -1, -4
F = np.float32
TABLE6 = np.array([254, 180, 110, 70, 55, 50], np.uint8)
TABLE1 = np.array([1], np.uint8)
VARIANTS = [(1, TABLE6), (5, TABLE1), (1, TABLE1), (5, TABLE6)]   # (min_clear_s2, table)


@pytest.fixture(scope="module")
def capi(lv):
    from limo_velo_amd import capi as c

    return c


def _grid_of(prm, mask):
    """Log-odds [nz, ny, nx]: occupied where mask, observed free elsewhere."""
    return np.where(mask, F(prm["l_max"]), F(prm["l_min"])).astype(F)


def _points(prm, dims, rng, n):
    """World points for goals and starts: cell centres, random ones in and round the field, non-finite and far ones."""
    lo = np.array(prm["origin"], np.float64)
    res = prm["resolution"]
    d = np.array(dims)
    centres = lo + (rng.integers(0, d, (n, 3)) + 0.5) * res
    odd = [[np.nan, lo[1], lo[2]], [lo[0], np.inf, lo[2]], [1e30, 0, 0], lo - 0.25 * res, lo + d * res + 0.25 * res]
    return np.concatenate([centres, rng.uniform(lo - res, lo + (d + 1) * res, (n // 2, 3)), odd]).astype(F)


def _all_centres(prm, dims):
    k, j, i = np.meshgrid(*(np.arange(n) for n in dims[::-1]), indexing="ij")
    return (np.array(prm["origin"]) + (np.stack([i, j, k], -1).reshape(-1, 3) + 0.5) * prm["resolution"]).astype(F)


def _hold(capi, ctx, prm, rs2, pp, table, goals, starts):
    """The GPU's plan over the distance field last built (the reference's: rs2) equals plan_ref's.  Returns (P, status, cells)."""
    rc, rP, rst, adj = pr.build(prm, rs2, pp, table, goals)
    st = ctx.occ_plan_build(goals, table, capi.default_plan_params(**pp))
    P, cc = ctx.occ_plan_fetch()
    assert cc.shape == rc.shape and np.array_equal(cc, rc), (pp, f"{np.sum(cc != rc)} cost bytes differ")
    assert np.array_equal(P, rP), (pp, f"{np.sum(P != rP)} potentials differ")
    assert list(st) == list(rst), (pp, st, rst)
    rstatus, rcost, roff, rcells = pr.paths(prm, rc, rP, adj, starts)
    status, cost, off, cells = ctx.occ_plan_paths(starts)
    assert np.array_equal(status, rstatus) and np.array_equal(cost, rcost) and np.array_equal(off, roff) and np.array_equal(cells, rcells), pp
    i = ctx.occ_plan_info()
    assert (i.built, i.stale, i.params.connectivity, i.params.min_clear_s2) == (1, 0, pp["connectivity"], pp["min_clear_s2"]) and i.rounds >= 1
    return P, status, cells


def _run_shape(capi, dims, planar, conns):
    nx, ny, nz = dims
    rng = np.random.default_rng(nx * 7 + ny * 3 + nz)
    prm = ocr.params(origin=(-1.0, 0.5, 2.0), resolution=0.25, nx=nx, ny=ny, nz=nz)
    fdims = (nx, ny, 1) if planar else dims
    dp = dr.dparams(planar=1, k_lo=0, k_hi=nz - 1) if planar else dr.dparams()
    small = nx * ny * (1 if planar else nz) <= 700
    starts = np.concatenate([_all_centres(prm, fdims), _points(prm, fdims, rng, 4)]) if small else _points(prm, fdims, rng, 60)
    goals5 = _points(prm, fdims, rng, 2)[[0, 1, 2, 3, 5]]   # two cell centres (may be obstacles), a random one, a NaN one, a far one
    n = 0
    with capi.Context() as ctx:
        ctx.occ_configure(capi.default_occupancy_params(**prm))
        for density in (0.0, 0.04, 0.2, 0.45):
            mask = rng.uniform(size=(nz, ny, nx)) < density
            if planar:
                mask[1:] = False   # (the band's projection is layer 0's obstacles)
            L = _grid_of(prm, mask)
            ctx.occ_load(L)
            ctx.occ_distance_build(capi.default_distance_params(**dp))
            rs2, _ = dr.build(prm, L, dp)
            for conn in conns:
                clear, table = VARIANTS[n % 4]
                goals = goals5 if n % 2 else goals5[:1]
                n += 1
                _hold(capi, ctx, prm, rs2, pr.pparams(connectivity=conn, min_clear_s2=clear), table, goals, starts)
        # every goal unusable: the build succeeds, nothing is reached
        P, status, _ = _hold(capi, ctx, prm, rs2, pr.pparams(connectivity=conns[0]), TABLE6, goals5[3:], starts)
        assert np.all(P == pr.UNREACHED) and not np.any(status == 0)


# ---- 1. shapes x densities x connectivities
@pytest.mark.parametrize("dims", [(1, 1), (1, 5), (31, 2), (33, 5), (65, 4), (1024, 2), (2, 1024)])
def test_planar_fields(capi, dims):
    _run_shape(capi, dims + (2,), True, (4, 8))


@pytest.mark.parametrize("dims", [(1, 5, 3), (9, 9, 9), (17, 9, 10), (33, 5, 3), (20, 7, 1)])
def test_3d_fields(capi, dims):
    _run_shape(capi, dims, False, (6, 18, 26))


# ---- 1b. goals on tile seams: a goal cell is never lowered, so the tiles that see it in their halo have to be woken by the seeding
SEAMS = [   # (nx, ny, nz), planar, goal cell, blocked cells
    ((64, 1, 1), True, (32, 0, 0), []), ((64, 1, 1), True, (31, 0, 0), []), ((1, 64, 1), True, (0, 32, 0), []), ((1, 64, 1), True, (0, 31, 0), []),
    ((17, 1, 1), False, (8, 0, 0), []), ((17, 1, 1), False, (7, 0, 0), []), ((1, 17, 1), False, (0, 8, 0), []), ((1, 1, 17), False, (0, 0, 7), []),
    ((33, 5, 1), True, (32, 2, 0), [(32, 1, 0), (32, 3, 0)]), ((33, 5, 1), True, (31, 2, 0), [(31, 1, 0), (31, 3, 0), (30, 1, 0), (30, 2, 0), (30, 3, 0)]),
    ((34, 34, 1), True, (31, 31, 0), [(30, 30, 0), (31, 30, 0), (30, 31, 0)]), ((34, 34, 1), True, (32, 32, 0), [(33, 33, 0), (32, 33, 0), (33, 32, 0)]),
    ((9, 9, 9), False, (7, 7, 7), [(i, j, k) for i in (6, 7) for j in (6, 7) for k in (6, 7) if (i, j, k) != (7, 7, 7)]),
    ((9, 9, 9), False, (8, 8, 8), []), ((17, 9, 10), False, (8, 7, 8), [(9, 7, 8), (8, 6, 8), (8, 7, 9), (9, 6, 8), (9, 7, 9), (8, 6, 9), (9, 6, 9)]),
]


@pytest.mark.parametrize("case", SEAMS, ids=lambda c: "%dx%dx%d-%s-goal%d.%d.%d" % (c[0] + ("planar" if c[1] else "3d",) + c[2]))
def test_goals_on_tile_seams(capi, case):
    (nx, ny, nz), planar, goal, blocked = case
    prm = ocr.params(origin=(-1.0, 0.5, 2.0), resolution=0.25, nx=nx, ny=ny, nz=nz)
    mask = np.zeros((nz, ny, nx), bool)
    for i, j, k in blocked:
        mask[k, j, i] = True
    L = _grid_of(prm, mask)
    dp = dr.dparams(planar=1, k_lo=0, k_hi=0) if planar else dr.dparams()
    rs2, _ = dr.build(prm, L, dp)
    goals = (np.array(prm["origin"]) + (np.array([goal]) + 0.5) * 0.25).astype(F)
    starts = _all_centres(prm, (nx, ny, nz))
    with capi.Context() as ctx:
        ctx.occ_configure(capi.default_occupancy_params(**prm))
        ctx.occ_load(L)
        ctx.occ_distance_build(capi.default_distance_params(**dp))
        for conn in ((4, 8) if planar else (6, 18, 26)):
            P, status, _ = _hold(capi, ctx, prm, rs2, pr.pparams(connectivity=conn), TABLE6, goals, starts)
            assert np.all((P != pr.UNREACHED) == ~(mask[0] if planar else mask))   # every free cell is reached: the field is connected


# ---- 2. a route that crosses the tile seams many times
def test_serpentine(capi):
    nx = ny = 70
    prm = ocr.params(origin=(0.0, 0.0, 0.0), resolution=0.5, nx=nx, ny=ny, nz=1)
    mask = np.zeros((1, ny, nx), bool)
    for r, j in enumerate(range(3, ny, 4)):   # walls on every fourth row, the gap at alternating ends
        mask[0, j, :] = True
        gap = slice(nx - 2, nx) if r % 2 == 0 else slice(0, 2)
        mask[0, j, gap] = False
    L = _grid_of(prm, mask)
    dp = dr.dparams(planar=1, k_lo=0, k_hi=0)
    rs2, _ = dr.build(prm, L, dp)
    goal = np.array([[0.25, 0.25, 0.0]], F)
    starts = np.array([[0.25, 34.75, 0.0], [34.75, 34.75, 0.0], [0.25, 0.25, 0.0], [10.25, 1.75, 0.0]], F)   # the far end, ..., the goal, a wall
    with capi.Context() as ctx:
        ctx.occ_configure(capi.default_occupancy_params(**prm))
        ctx.occ_load(L)
        ctx.occ_distance_build(capi.default_distance_params(**dp))
        for conn in (4, 8):
            P, status, cells = _hold(capi, ctx, prm, rs2, pr.pparams(connectivity=conn), TABLE6, goal, starts)
            assert list(status) == [0, 0, 0, 2]
            assert P[ny - 1, 0] != pr.UNREACHED and np.all((P != pr.UNREACHED) == ~mask[0])
            off = ctx.occ_plan_paths(starts)[2]
            assert off[1] > 17 * (nx - 4)   # the route runs the length of every corridor
            assert off[3] - off[2] == 1 and cells[int(off[2])] == 0   # a start on the goal: one cell
            assert ctx.occ_plan_info().rounds > 17   # more rounds than a tile-by-tile flood of open space would take


# ---- 3. pockets, the kinds of start, determinism, capacity
def _pocket_case():
    nx, ny = 40, 36
    prm = ocr.params(origin=(-2.0, 1.0, 0.0), resolution=0.25, nx=nx, ny=ny, nz=3)
    mask = np.zeros((3, ny, nx), bool)
    mask[0, 10:17, 30] = mask[0, 10:17, 36] = True   # a walled pocket across the tile seam at x = 32
    mask[0, 10, 30:37] = mask[0, 16, 30:37] = True
    mask[2, 3, 3] = True                             # an obstacle in another layer of the band
    L = _grid_of(prm, mask)
    dp = dr.dparams(planar=1, k_lo=0, k_hi=2)
    lo, res = np.array(prm["origin"]), 0.25
    cell = lambda i, j: lo + (np.array([i, j, 0]) + 0.5) * res
    goals = np.array([cell(2, 30), cell(30, 10), [np.nan, 0, 0], cell(-3, 2), cell(20, 2)], F)   # free, a wall, NaN, outside, free
    starts = np.array([cell(33, 13), cell(30, 12), cell(45, 3), [0, np.inf, 0], cell(2, 30), cell(3, 3), cell(25, 20)], F)
    starts[6, 2] = np.nan   # (z is not looked at)
    return prm, L, dp, goals, starts


def test_pockets_starts_determinism_and_capacity(capi):
    prm, L, dp, goals, starts = _pocket_case()
    rs2, _ = dr.build(prm, L, dp)
    pp = pr.pparams(connectivity=8, min_clear_s2=1)
    with capi.Context() as ctx:
        ctx.occ_configure(capi.default_occupancy_params(**prm))
        ctx.occ_load(L)
        ctx.occ_distance_build(capi.default_distance_params(**dp))
        P, status, cells = _hold(capi, ctx, prm, rs2, pp, TABLE6, goals, starts)
        assert list(status) == [1, 2, 2, 2, 0, 2, 0]   # in the pocket, in a wall, outside, non-finite, on a goal, an obstacle, free
        assert P[13, 33] == pr.UNREACHED and P[30, 2] == 0 and P[2, 20] == 0
        st, cost, off, _ = ctx.occ_plan_paths(starts)
        assert off[5] - off[4] == 1 and cost[4] == 0 and cost[0] == pr.UNREACHED
        # two builds of the same input: the same bits
        first = [a.copy() for a in ctx.occ_plan_fetch()] + [a.copy() for a in ctx.occ_plan_paths(starts)]
        ctx.occ_plan_build(goals, TABLE6, capi.default_plan_params(**pp))
        again = list(ctx.occ_plan_fetch()) + list(ctx.occ_plan_paths(starts))
        assert all(np.array_equal(a, b) for a, b in zip(first, again))
        # count only, then a capacity one short: LV_EINVAL with status, cost, offsets and total written, cells untouched
        lib, h = ctx.lib, ctx.h
        n = len(starts)
        total = int(off[-1])
        s2_, c2, o2 = np.full(n, 7, np.int32), np.full(n, 7, np.uint32), np.full(n + 1, 7, np.uint64)
        t = C.c_size_t(0)
        buf = np.full(total, -5, np.int32)
        args = (h, starts.ctypes.data_as(C.c_void_p), 12, n, s2_.ctypes.data_as(C.POINTER(C.c_int32)), c2.ctypes.data_as(C.POINTER(C.c_uint32)),
                o2.ctypes.data_as(C.POINTER(C.c_size_t)))
        assert lib.lv_occ_plan_paths(*args, None, 0, C.byref(t)) == 0 and t.value == total
        assert np.array_equal(s2_, st) and np.array_equal(c2, cost) and np.array_equal(o2, off)
        o2[:] = 7
        t.value = 0
        assert lib.lv_occ_plan_paths(*args, buf.ctypes.data_as(C.POINTER(C.c_int32)), total - 1, C.byref(t)) == LV_EINVAL
        assert t.value == total and np.array_equal(o2, off) and np.all(buf == -5)
        assert lib.lv_occ_plan_paths(*args, buf.ctypes.data_as(C.POINTER(C.c_int32)), total, C.byref(t)) == 0 and np.array_equal(buf, cells)
        # no starts at all
        assert lib.lv_occ_plan_paths(h, None, 12, 0, None, None, o2.ctypes.data_as(C.POINTER(C.c_size_t)), None, 0, C.byref(t)) == 0
        assert t.value == 0 and o2[0] == 0
        # fetch: one output, both NULL, a capacity one short
        pot, none = ctx.occ_plan_fetch(cell_cost=False)
        assert none is None and np.array_equal(pot, P)
        none, cc = ctx.occ_plan_fetch(potential=False)
        assert none is None and np.array_equal(cc, first[1])
        assert lib.lv_occ_plan_fetch(h, None, None, P.size) == LV_EINVAL
        small = np.full(P.size, 9, np.uint32)
        assert lib.lv_occ_plan_fetch(h, small.ctypes.data_as(C.POINTER(C.c_uint32)), None, P.size - 1) == LV_EINVAL and np.all(small == 9)


def test_the_python_helpers(capi):
    from limo_velo_amd import occupancy

    prm, L, dp, goals, starts = _pocket_case()
    rs2, _ = dr.build(prm, L, dp)
    with capi.Context() as ctx:
        ctx.occ_configure(capi.default_occupancy_params(**prm))
        ctx.occ_load(L)
        ctx.occ_distance_build(capi.default_distance_params(**dp))
        info, st = occupancy.plan(ctx, goals, robot_radius=0.3, inflation_radius=1.0)
        table = occupancy.inflation_cost_table(0.25, 0.3, 1.0)
        clear = occupancy.min_clear_s2(0.25, 0.3)
        assert clear == 2 and (info.built, info.planar, info.nx, info.ny, info.nz, info.params.connectivity, info.params.min_clear_s2) == (1, 1, 40, 36, 1, 8, 2)
        rc, rP, rst, adj = pr.build(prm, rs2, pr.pparams(min_clear_s2=clear), table, goals)
        assert list(st) == list(rst) and np.array_equal(ctx.occ_plan_fetch()[0], rP)
        rstatus, rcost, roff, rcells = pr.paths(prm, rc, rP, adj, starts)
        got = occupancy.routes(ctx, starts)
        assert [s for _, s, _ in got] == list(rstatus) and [c for _, _, c in got] == list(rcost)
        for s, (line, status, _) in enumerate(got):
            row = rcells[int(roff[s]):int(roff[s + 1])].astype(np.int64)
            want = np.stack([-2.0 + (row % 40 + 0.5) * 0.25, 1.0 + (row // 40 + 0.5) * 0.25], axis=1).astype(F)
            assert line.shape == (len(row), 2) and np.array_equal(line, want)


# ---- 4. lifecycle
def test_lifecycle(capi):
    prm, L, dp, goals, starts = _pocket_case()
    rs2, _ = dr.build(prm, L, dp)
    pp = pr.pparams()
    rc, rP, rst, adj = pr.build(prm, rs2, pp, TABLE6, goals)
    want = pr.paths(prm, rc, rP, adj, starts)
    with capi.Context() as ctx:
        lib, h = ctx.lib, ctx.h
        info = capi.PlanInfo()
        cpp = capi.default_plan_params(**pp)
        u8, u32, i32, sz = C.POINTER(C.c_uint8), C.POINTER(C.c_uint32), C.POINTER(C.c_int32), C.POINTER(C.c_size_t)
        g = np.ascontiguousarray(goals)
        stats = np.full(4, 7, np.uint64)
        buf = np.full(8, 3, np.uint32)
        off = np.full(2, 3, np.uint64)
        st = np.full(1, 3, np.int32)
        t = C.c_size_t(3)

        def build(p=cpp):
            return lib.lv_occ_plan_build(h, C.byref(p), TABLE6.ctypes.data_as(u8), 6, g.ctypes.data_as(C.c_void_p), 12, len(g),
                                         stats.ctypes.data_as(C.POINTER(C.c_uint64)))

        def fetch_and_paths():
            return (lib.lv_occ_plan_fetch(h, buf.ctypes.data_as(u32), None, 8),
                    lib.lv_occ_plan_paths(h, g.ctypes.data_as(C.c_void_p), 12, 1, st.ctypes.data_as(i32), buf.ctypes.data_as(u32),
                                          off.ctypes.data_as(sz), None, 0, C.byref(t)))

        # before lv_occ_configure
        assert build() == LV_ESTATE and fetch_and_paths() == (LV_ESTATE, LV_ESTATE)
        assert lib.lv_occ_plan_info(h, C.byref(info)) == LV_ESTATE and lib.lv_occ_plan_clear(h) == LV_ESTATE
        # configured, before a distance build; then before a plan build
        ctx.occ_configure(capi.default_occupancy_params(**prm))
        ctx.occ_load(L)
        assert build() == LV_ESTATE and fetch_and_paths() == (LV_ESTATE, LV_ESTATE)
        ctx.occ_distance_build(capi.default_distance_params(**dp))
        assert fetch_and_paths() == (LV_ESTATE, LV_ESTATE)
        i = ctx.occ_plan_info()
        assert (i.built, i.planar, i.nx, i.ny, i.nz, i.stale, i.rounds) == (0, 0, 0, 0, 0, 0, 0)
        ctx.occ_plan_clear()   # (nothing to free: fine)
        # a connectivity that does not suit the field: refused, nothing built, nothing written
        assert build(capi.default_plan_params(connectivity=26)) == LV_EINVAL and ctx.occ_plan_info().built == 0
        assert np.all(stats == 7) and np.all(buf == 3) and np.all(off == 3) and st[0] == 3 and t.value == 3
        assert build() == 0 and list(stats) == list(rst)
        i = ctx.occ_plan_info()
        assert (i.built, i.planar, i.nx, i.ny, i.nz, i.stale) == (1, 1, 40, 36, 1, 0)
        # a refused build leaves the plan in place
        assert build(capi.default_plan_params(connectivity=6)) == LV_EINVAL and build(capi.default_plan_params(min_clear_s2=0)) == LV_EINVAL
        assert np.array_equal(ctx.occ_plan_fetch()[0], rP)
        # the distance field moves on, the snapshot stays: after a rebuild (here 3-D, another size) and after a clear
        for change in (lambda: ctx.occ_distance_build(capi.default_distance_params(unknown_is_obstacle=1)), ctx.occ_distance_clear):
            assert build() == 0 and ctx.occ_plan_info().stale == 0
            change()
            i = ctx.occ_plan_info()
            assert (i.built, i.stale, i.planar, i.nz) == (1, 1, 1, 1)
            P, cc = ctx.occ_plan_fetch()
            assert np.array_equal(P, rP) and np.array_equal(cc, rc)
            assert all(np.array_equal(a, b) for a, b in zip(ctx.occ_plan_paths(starts), want))
            ctx.occ_distance_build(capi.default_distance_params(**dp))
        # the grid changing makes the FIELD stale, not the plan; a stale field is planned on as it is
        assert build() == 0
        ctx.occ_clear()
        assert ctx.occ_distance_info().stale == 1 and ctx.occ_plan_info().stale == 0
        assert build() == 0 and np.array_equal(ctx.occ_plan_fetch()[0], rP)
        # a 3-D field takes 6, 18 or 26 and refuses the default 8
        ctx.occ_load(L)
        ctx.occ_distance_build(capi.default_distance_params())
        assert build() == LV_EINVAL and ctx.occ_plan_info().planar == 1
        assert build(capi.default_plan_params(connectivity=18)) == 0
        i = ctx.occ_plan_info()
        assert (i.built, i.planar, i.nx, i.ny, i.nz, i.stale, i.params.connectivity) == (1, 0, 40, 36, 3, 0, 18)
        # lv_occ_plan_clear discards it; so does lv_occ_configure (a refused one does not)
        ctx.occ_plan_clear()
        assert ctx.occ_plan_info().built == 0 and fetch_and_paths() == (LV_ESTATE, LV_ESTATE)
        assert build(capi.default_plan_params(connectivity=6)) == 0
        badgrid = capi.default_occupancy_params(**dict(prm, nx=1025))
        assert lib.lv_occ_configure(h, C.byref(badgrid)) == LV_EINVAL and ctx.occ_plan_info().built == 1
        ctx.occ_configure(capi.default_occupancy_params(**dict(prm, nx=44)))
        assert ctx.occ_plan_info().built == 0 and fetch_and_paths() == (LV_ESTATE, LV_ESTATE)


# ---- 5. untouched state
def test_the_grid_the_field_the_map_and_the_update_are_untouched(capi):
    from limo_velo_amd import synth

    sc = synth.make_ring_scene(20_000, 16, 256)
    prm, L, dp, goals, starts = _pocket_case()
    with capi.Context() as ctx:
        ctx.map_build(sc["map_xyz"])
        ctx.scan_set(sc["scan_xyz"])
        x0, P0, passes0, _, _ = ctx.update(sc["x_init"], sc["P0"])
        x0, P0 = np.array(x0), np.array(P0)
        stats0 = ctx.map_stats()
        ctx.occ_configure(capi.default_occupancy_params(**prm))
        ctx.occ_load(L)
        before = ctx.occ_fetch()
        for d, conn in ((dp, 8), (dr.dparams(signed_field=1), 26)):
            ctx.occ_distance_build(capi.default_distance_params(**d))
            s2, met = ctx.occ_distance_fetch()
            ctx.occ_plan_build(goals, TABLE6, capi.default_plan_params(connectivity=conn))
            ctx.occ_plan_fetch()
            ctx.occ_plan_paths(starts)
            assert np.array_equal(ctx.occ_fetch().view(np.uint32), before.view(np.uint32))
            s2b, metb = ctx.occ_distance_fetch()
            assert np.array_equal(s2b, s2) and np.array_equal(metb.view(np.uint32), met.view(np.uint32)) and ctx.occ_distance_info().stale == 0
        x1, P1, passes1, _, _ = ctx.update(sc["x_init"], sc["P0"])
        assert passes1 == passes0
        assert np.array_equal(np.array(x1).view(np.uint64), x0.view(np.uint64))
        assert np.array_equal(np.array(P1).view(np.uint64), P0.view(np.uint64))
        assert ctx.map_stats() == stats0
