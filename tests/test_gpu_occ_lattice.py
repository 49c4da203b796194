"""GPU tests of the lattice planner (lv_lattice.hip; include/limovelo_hip.h "Lattice planner") against the statement of the rule in
tests/lattice_ref.py.  Edge costs are integers and V is the unique fixpoint of relaxation, so everything is held to equality on every
state and every path: V, stats, status, path costs, offsets, path states and the primitives taken.  The grids are set with occ_load,
then the planar distance field, then the plan, as tests/test_gpu_occ_plan.py does; the cost bytes the reference runs on are plan_ref's."""
import ctypes as C

import numpy as np
import pytest

import distance_ref as dr
import lattice_ref as lr
import occupancy_ref as ocr
import plan_ref as pr

pytestmark = pytest.mark.gpu

LV_EINVAL, LV_ESTATE = -1, -4
F = np.float32
TABLE6 = np.array([254, 180, 110, 70, 55, 50], np.uint8)
TABLE1 = np.array([1], np.uint8)
TABLE255 = np.array([255], np.uint8)
DP = dict(planar=1, k_lo=0, k_hi=0)


@pytest.fixture(scope="module")
def capi(lv):
    from limo_velo_amd import capi as c

    return c


def _params(nx, ny, origin=(-1.0, 0.5, 2.0), resolution=0.25, nz=1):
    return ocr.params(origin=origin, resolution=resolution, nx=nx, ny=ny, nz=nz)


def _centre(prm, i, j, h, z=0.0):
    return [prm["origin"][0] + (i + 0.5) * prm["resolution"], prm["origin"][1] + (j + 0.5) * prm["resolution"], z, h]


def _plan(capi, ctx, prm, mask, table=TABLE6, clear=1, configure=True):
    """The grid (occupied where mask [ny, nx]), its planar field and a plan on the device; returns plan_ref's cost bytes [ny, nx]."""
    L = np.where(mask[None], F(prm["l_max"]), F(prm["l_min"])).astype(F)
    if configure:
        ctx.occ_configure(capi.default_occupancy_params(**prm))
    ctx.occ_load(L)
    ctx.occ_distance_build(capi.default_distance_params(**DP))
    rs2, _ = dr.build(prm, L, dr.dparams(**DP))
    ctx.occ_plan_build(np.array([_centre(prm, 0, 0, 0)[:3]], F), table, capi.default_plan_params(connectivity=8, min_clear_s2=clear))
    return pr.cell_cost(rs2, clear, table)


def _pose_set(prm, dims, H, rng, n):
    """Goal and start records: cell centres with every kind of heading, random points in and round the grid, non-finite and far ones."""
    nx, ny = dims
    lo, res = np.array(prm["origin"], np.float64), prm["resolution"]
    rows = [_centre(prm, int(rng.integers(nx)), int(rng.integers(ny)), int(h), rng.uniform()) for h in list(rng.integers(-1, H, n)) + [-1, 0, H - 1, H, -2]]
    rows += [[rng.uniform(lo[0] - res, lo[0] + (nx + 1) * res), rng.uniform(lo[1] - res, lo[1] + (ny + 1) * res), np.nan, int(rng.integers(-1, H))] for _ in range(n // 2)]
    rows += [[np.nan, lo[1], 0, 0], [lo[0], np.inf, 0, -1], [1e30, 0, 0, 0], [lo[0] - 0.25 * res, lo[1], 0, 0]]
    return lr.poses(rows)


def _all_cells(prm, dims, h=-1):
    return lr.poses([_centre(prm, i, j, h) for j in range(dims[1]) for i in range(dims[0])])


def _hold(ctx, prm, c, t, goals, starts, tile=None):
    """The GPU's lattice over the plan last built (cost bytes c) equals lattice_ref's.  Returns (V, status, cost, off, states, taken)."""
    H, P = t.shape
    rV, rst = lr.build(prm, c, t, goals)
    st = ctx.occ_lattice_build(goals, t)
    V = ctx.occ_lattice_fetch()
    assert V.shape == rV.shape and np.array_equal(V, rV), f"{np.sum(V != rV)} of {V.size} states differ"
    assert list(st) == list(rst), (st, rst)
    want = lr.paths(prm, c, rV, t, starts)
    got = ctx.occ_lattice_paths(starts)
    assert all(np.array_equal(a, b) for a, b in zip(got, want))
    i = ctx.occ_lattice_info()
    assert (i.built, i.nx, i.ny, i.H, i.P, i.stale, i.reach, i.params.H, i.params.P) == (1, c.shape[1], c.shape[0], H, P, 0, lr.reach_of(t), H, P)
    assert i.rounds >= 1 and (tile is None or i.tile == tile)
    return (V,) + tuple(got)


def _table_8_3(rng):
    """H = 8, P = 3, reach 1..2: takes the tile of edge 16."""
    t = lr.random_table(rng, 8, 3, 2)
    t[0, 0] = lr.prim(2, -1, 1, 17, 3, [(1, 0)])
    return t


def _table_16_reach8(rng, P=4):
    """H = 16 with a reach of 8: takes the tile of edge 8."""
    t = lr.random_table(rng, 16, P, 8)
    t[3, 1] = lr.prim(8, -8, 5, 29, 1, [(4, -4)])
    t[9, 0] = lr.prim(-8, 3, 9, 21)
    return t


# ---- 1. shapes x densities x cost tables x both tile instantiations
@pytest.mark.parametrize("dims", [(37, 29), (70, 45), (1, 1), (1, 40)])
def test_shapes_densities_and_both_tiles(capi, dims):
    nx, ny = dims
    rng = np.random.default_rng(nx * 7 + ny * 3)
    prm = _params(nx, ny)
    seen = set()
    with capi.Context() as ctx:
        ctx.occ_configure(capi.default_occupancy_params(**prm))
        for n, density in enumerate((0.0, 0.04, 0.2, 0.45)):
            mask = rng.uniform(size=(ny, nx)) < density
            table, clear = ((TABLE6, 1), (TABLE1, 2))[n % 2]
            c = _plan(capi, ctx, prm, mask, table, clear, configure=False)
            for make, H, tile in ((_table_8_3, 8, 16), (_table_16_reach8, 16, 8)):
                t = make(rng)
                ps = _pose_set(prm, dims, H, rng, 10)
                starts = np.concatenate([ps, _all_cells(prm, dims)]) if nx * ny <= 1200 else ps
                out = _hold(ctx, prm, c, t, ps[:6], starts, tile)
                seen |= set(out[1].tolist())
        # every goal unusable: the build succeeds, nothing is reached
        V, status = _hold(ctx, prm, c, t, ps[-4:], starts)[:2]
        assert np.all(V == lr.UNREACHED) and not np.any(status == 0)
    assert 2 in seen and (nx * ny == 1 or 0 in seen)


# ---- 2. a jump of 8 cells over a wall: the only way across, and it crosses tile seams
@pytest.mark.parametrize("sign", [1, -1])
def test_the_only_way_across_a_wall_is_a_jump_of_eight(capi, sign):
    nx, ny, H = 41, 19, 16
    prm = _params(nx, ny)
    mask = np.zeros((ny, nx), bool)
    mask[:, 17:24] = True   # seven columns: a step of one never crosses, a jump of eight does
    h = 0 if sign > 0 else 8
    t = lr.table(H, 4)
    t[h, 0] = lr.prim(8 * sign, 0, h, 30, 0, [(4 * sign, 0)])   # the cheaper jump looks at a cell of the wall: never allowed where it matters
    t[h, 1] = lr.prim(sign, 0, h, 10)
    t[h, 2] = lr.prim(0, 0, (h + 1) % H, 0)                      # an empty slot
    t[h, 3] = lr.prim(8 * sign, 0, h, 90, 5)                    # the jump: its ends only
    gi, si = (nx - 2, 1) if sign > 0 else (1, nx - 2)
    goals = lr.poses([_centre(prm, gi, 9, h)])
    with capi.Context() as ctx:
        c = _plan(capi, ctx, prm, mask)
        V, status, cost, off, states, taken = _hold(ctx, prm, c, t, goals, np.concatenate([lr.poses([_centre(prm, si, 9, h)]), _all_cells(prm, (nx, ny), h)]), tile=8)
        assert status[0] == 0 and V[h, 9, si] != lr.UNREACHED and list(taken[int(off[0]):int(off[1])]).count(3) == 1
        far = V[h, :, :17] if sign > 0 else V[h, :, 24:]
        assert np.any(far[9] != lr.UNREACHED) and ctx.occ_lattice_info().rounds >= 3


# ---- 3. directed edges: a dead end that only reversing gets out of
def test_a_dead_end_needs_reversing(capi):
    nx = 20
    prm = _params(nx, 1)
    fwd = lr.table(2, 2)
    fwd[0, 0] = lr.prim(1, 0, 0, 10)
    fwd[1, 0] = lr.prim(-1, 0, 1, 10)
    rev = fwd.copy()
    rev[0, 1] = lr.prim(-1, 0, 0, 10, 200)
    rev[1, 1] = lr.prim(1, 0, 1, 10, 200)
    goals = lr.poses([_centre(prm, 3, 0, -1)])
    starts = lr.poses([_centre(prm, nx - 1, 0, 0), _centre(prm, nx - 1, 0, 1), _centre(prm, 0, 0, 0)])   # facing the wall, facing the goal, before it
    with capi.Context() as ctx:
        c = _plan(capi, ctx, prm, np.zeros((1, nx), bool), TABLE1)
        _, status, cost = _hold(ctx, prm, c, fwd, goals, starts, tile=16)[:3]
        assert list(status) == [1, 0, 0] and list(cost) == [lr.UNREACHED, 16 * 20, 3 * 20]
        _, status, cost = _hold(ctx, prm, c, rev, goals, starts)[:3]
        assert list(status) == [0, 0, 0] and list(cost) == [16 * (20 + 200), 16 * 20, 3 * 20]


# ---- 4. one heading and the planner's eight moves: the device's own plan
@pytest.mark.parametrize("dims", [(37, 29), (70, 45)])
def test_one_heading_is_the_devices_own_plan(capi, dims):
    nx, ny = dims
    rng = np.random.default_rng(nx + ny)
    prm = _params(nx, ny)
    t = lr.neighbour_table()
    with capi.Context() as ctx:
        for density in (0.0, 0.2, 0.45):
            c = _plan(capi, ctx, prm, rng.uniform(size=(ny, nx)) < density)
            pts = np.array([_centre(prm, int(rng.integers(nx)), int(rng.integers(ny)), 0)[:3] for _ in range(3)], F)
            ctx.occ_plan_build(pts, TABLE6, capi.default_plan_params(connectivity=8))
            P, cc = ctx.occ_plan_fetch()
            assert np.array_equal(cc, c)
            goals = lr.poses(np.concatenate([pts, np.zeros((3, 1))], axis=1))
            ctx.occ_lattice_build(goals, t)
            assert np.array_equal(ctx.occ_lattice_fetch()[0], P) and ctx.occ_lattice_info().tile == 16
            _hold(ctx, prm, c, t, goals, _pose_set(prm, dims, 1, rng, 10))


# ---- 5. turns on the spot, sweeps that block, sums that reach the limit
def test_turns_on_the_spot_and_blocked_sweep_cells(capi):
    nx, ny = 9, 3
    prm = _params(nx, ny)
    mask = np.zeros((ny, nx), bool)
    mask[1, 4] = True
    t = lr.table(4, 3)
    t[0, 0] = lr.prim(2, 0, 0, 20, 0, [(1, 0)])   # two cells along +x, through the cell between
    t[0, 1] = lr.prim(0, 0, 1, 5, 2)             # turn on the spot
    t[1, 0] = lr.prim(0, 1, 1, 10)
    t[1, 1] = lr.prim(0, 0, 0, 5, 2)
    t[3, 2] = lr.prim(0, -1, 3, 10)
    t[0, 2] = lr.prim(0, 0, 3, 5, 2)
    t[3, 1] = lr.prim(0, 0, 0, 5, 2)
    goals = lr.poses([_centre(prm, 7, 1, 0)])
    starts = np.concatenate([_all_cells(prm, (nx, ny), h) for h in range(4)])
    with capi.Context() as ctx:
        c = _plan(capi, ctx, prm, mask, TABLE1)
        V = _hold(ctx, prm, c, t, goals, starts, tile=16)[0]
        # on the middle row, (3, 1) -> (5, 1) has both ends free and sweeps the obstacle: the way is round it by rows 0 or 2
        assert V[0, 1, 5] == 2 * 20 and V[0, 1, 3] not in (lr.UNREACHED, 2 * 20 * 2) and V[0, 1, 3] > 80


def test_sums_that_reach_the_limit(capi):
    nx = 100
    prm = _params(nx, 1, origin=(0.0, 0.0, 0.0), resolution=1.0)
    t = lr.table(1, 1)
    t[0, 0] = lr.prim(-1, 0, 0, 65535, 1 << 24)
    step = 65535 * 510 + (1 << 24)
    n = (lr.UNREACHED - 1) // step
    with capi.Context() as ctx:
        c = _plan(capi, ctx, prm, np.zeros((1, nx), bool), TABLE255)
        assert np.all(c == 255)
        V, status, cost = _hold(ctx, prm, c, t, lr.poses([[0.5, 0.5, 0, 0]]), lr.poses([[n + 0.5, 0.5, 0, 0], [n + 1.5, 0.5, 0, 0]]))[:3]
        assert list(V[0, 0, :n + 1]) == [k * step for k in range(n + 1)] and np.all(V[0, 0, n + 1:] == lr.UNREACHED)
        assert list(status) == [0, 1] and cost[0] == n * step


# ---- 6. CSR output
def test_csr_count_only_capacity_and_prims(capi):
    nx, ny = 37, 29
    rng = np.random.default_rng(5)
    prm = _params(nx, ny)
    t = _table_8_3(rng)
    ps = _pose_set(prm, (nx, ny), 8, rng, 20)
    with capi.Context() as ctx:
        c = _plan(capi, ctx, prm, rng.uniform(size=(ny, nx)) < 0.1)
        _, status, cost, off, states, taken = _hold(ctx, prm, c, t, ps[:8], ps)
        lib, h = ctx.lib, ctx.h
        n, total = len(ps), int(off[-1])
        assert total > 0
        s2, c2, o2 = np.full(n, 7, np.int32), np.full(n, 7, np.uint32), np.full(n + 1, 7, np.uint64)
        tt = C.c_size_t(0)
        buf, pb = np.full(total, -5, np.int32), np.full(total, 9, np.uint8)
        i32, u8 = C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
        args = (h, ps.ctypes.data_as(C.c_void_p), 16, n, s2.ctypes.data_as(i32), c2.ctypes.data_as(C.POINTER(C.c_uint32)), o2.ctypes.data_as(C.POINTER(C.c_size_t)))
        assert lib.lv_occ_lattice_paths(*args, None, pb.ctypes.data_as(u8), 0, C.byref(tt)) == 0 and tt.value == total   # count only
        assert np.array_equal(s2, status) and np.array_equal(c2, cost) and np.array_equal(o2, off) and np.all(pb == 9)
        o2[:] = 7
        tt.value = 0
        assert lib.lv_occ_lattice_paths(*args, buf.ctypes.data_as(i32), pb.ctypes.data_as(u8), total - 1, C.byref(tt)) == LV_EINVAL   # short by one
        assert tt.value == total and np.array_equal(o2, off) and np.all(buf == -5) and np.all(pb == 9)
        assert lib.lv_occ_lattice_paths(*args, buf.ctypes.data_as(i32), None, total, C.byref(tt)) == 0 and np.array_equal(buf, states) and np.all(pb == 9)
        buf[:] = -5
        assert lib.lv_occ_lattice_paths(*args, buf.ctypes.data_as(i32), pb.ctypes.data_as(u8), total, C.byref(tt)) == 0
        assert np.array_equal(buf, states) and np.array_equal(pb, taken)
        assert lib.lv_occ_lattice_paths(h, None, 16, 0, None, None, o2.ctypes.data_as(C.POINTER(C.c_size_t)), None, None, 0, C.byref(tt)) == 0   # no starts
        assert tt.value == 0 and o2[0] == 0
        assert lib.lv_occ_lattice_paths(*args[:2], 12, *args[3:], None, None, 0, C.byref(tt)) == LV_EINVAL   # a stride below 16
        small = np.full(V_size := 8 * ny * nx, 9, np.uint32)
        assert lib.lv_occ_lattice_fetch(h, small.ctypes.data_as(C.POINTER(C.c_uint32)), V_size - 1) == LV_EINVAL and np.all(small == 9)
        assert lib.lv_occ_lattice_fetch(h, None, V_size) == LV_EINVAL


# ---- 7. lifecycle
def test_lifecycle(capi):
    nx, ny = 37, 29
    rng = np.random.default_rng(11)
    prm = _params(nx, ny, nz=3)
    t = _table_8_3(rng)
    ps = _pose_set(prm, (nx, ny), 8, rng, 12)
    g = np.ascontiguousarray(ps[:6])
    mask = rng.uniform(size=(ny, nx)) < 0.1
    with capi.Context() as ctx:
        lib, h = ctx.lib, ctx.h
        info = capi.LatticeInfo()
        stats = np.full(4, 7, np.uint64)
        buf = np.full(8, 3, np.uint32)
        off = np.full(2, 3, np.uint64)
        st = np.full(1, 3, np.int32)
        tt = C.c_size_t(3)

        def build(table=t, H=8, P=3, goals=g, n_goals=None, ctx_h=h, n_prims=None):
            p = capi.LatticeParams(H, P)
            tab = np.ascontiguousarray(table)
            return lib.lv_occ_lattice_build(ctx_h, C.byref(p), tab.ctypes.data_as(C.POINTER(capi.LatticePrim)), tab.size if n_prims is None else n_prims,
                                            goals.ctypes.data_as(C.c_void_p), 16, len(goals) if n_goals is None else n_goals,
                                            stats.ctypes.data_as(C.POINTER(C.c_uint64)))

        def fetch_and_paths():
            return (lib.lv_occ_lattice_fetch(h, buf.ctypes.data_as(C.POINTER(C.c_uint32)), 8),
                    lib.lv_occ_lattice_paths(h, g.ctypes.data_as(C.c_void_p), 16, 1, st.ctypes.data_as(C.POINTER(C.c_int32)), buf.ctypes.data_as(C.POINTER(C.c_uint32)),
                                             off.ctypes.data_as(C.POINTER(C.c_size_t)), None, None, 0, C.byref(tt)))

        # before lv_occ_configure; what is judged before the context comes first, "null context" last
        assert build() == LV_ESTATE and fetch_and_paths() == (LV_ESTATE, LV_ESTATE)
        assert lib.lv_occ_lattice_info(h, C.byref(info)) == LV_ESTATE and lib.lv_occ_lattice_clear(h) == LV_ESTATE
        bad = t.copy()
        bad[2, 1]["reserved"] = 1
        for kw in (dict(H=0), dict(H=17), dict(P=17), dict(n_prims=23), dict(table=bad), dict(table=lr.table(8, 3)), dict(n_goals=0), dict(n_goals=65537)):
            assert build(**kw) == LV_EINVAL and build(ctx_h=None, **kw) == LV_EINVAL, kw
            assert b"null context" not in lib.lv_last_error()
        assert build(table=bad) == LV_EINVAL and b"record 7" in lib.lv_last_error()
        assert build(ctx_h=None) == LV_EINVAL and b"null context" in lib.lv_last_error()
        # configured, before a field; with a field, before a plan
        ctx.occ_configure(capi.default_occupancy_params(**prm))
        assert build() == LV_ESTATE and b"no plan" in lib.lv_last_error() and fetch_and_paths() == (LV_ESTATE, LV_ESTATE)
        i = ctx.occ_lattice_info()
        assert (i.built, i.nx, i.ny, i.H, i.P, i.stale, i.rounds, i.tile, i.reach) == (0,) * 9
        ctx.occ_lattice_clear()   # (nothing to free: fine)
        L = np.where(np.stack([mask, np.zeros_like(mask), np.zeros_like(mask)]), F(prm["l_max"]), F(prm["l_min"])).astype(F)
        ctx.occ_load(L)
        ctx.occ_distance_build(capi.default_distance_params(**DP))
        assert build() == LV_ESTATE and b"no plan" in lib.lv_last_error()
        # a 3-D plan is refused
        ctx.occ_distance_build(capi.default_distance_params())
        goal3 = np.array([_centre(prm, 0, 0, 0)[:3]], F)
        ctx.occ_plan_build(goal3, TABLE6, capi.default_plan_params(connectivity=26))
        assert build() == LV_ESTATE and b"3-D" in lib.lv_last_error() and ctx.occ_lattice_info().built == 0
        assert np.all(stats == 7) and np.all(buf == 3) and np.all(off == 3) and st[0] == 3 and tt.value == 3   # refused calls wrote nothing
        # the planar plan
        ctx.occ_distance_build(capi.default_distance_params(**DP))
        rs2, _ = dr.build(prm, L, dr.dparams(**DP))
        c = pr.cell_cost(rs2, 1, TABLE6)
        ctx.occ_plan_build(goal3, TABLE6, capi.default_plan_params(connectivity=8))
        V, status, cost, poff, states, taken = _hold(ctx, prm, c, t, ps[:6], ps, tile=16)
        want = (status, cost, poff, states, taken)

        def same():
            return np.array_equal(ctx.occ_lattice_fetch(), V) and all(np.array_equal(a, b) for a, b in zip(ctx.occ_lattice_paths(ps), want))

        # a refused build leaves the old lattice bit for bit
        assert build(table=bad) == LV_EINVAL and build(H=17) == LV_EINVAL and same() and ctx.occ_lattice_info().stale == 0
        # a distance rebuild or a grid edit does not touch it; a plan build (even a refused one past its own checks: none here) and a plan clear mark it stale
        ctx.occ_distance_build(capi.default_distance_params(**DP, unknown_is_obstacle=1))
        ctx.occ_clear()
        ctx.occ_load(L)
        assert ctx.occ_lattice_info().stale == 0 and ctx.occ_plan_info().stale == 1 and same()
        assert lib.lv_occ_plan_build(h, C.byref(capi.default_plan_params(connectivity=26)), TABLE6.ctypes.data_as(C.POINTER(C.c_uint8)), 6,
                                     goal3.ctypes.data_as(C.c_void_p), 12, 1, None) == LV_EINVAL   # refused by its own check: no plan edit
        assert ctx.occ_lattice_info().stale == 0
        ctx.occ_plan_build(goal3, TABLE1, capi.default_plan_params(connectivity=4))
        assert ctx.occ_lattice_info().stale == 1 and same()
        assert build() == 0 and ctx.occ_lattice_info().stale == 0
        ctx.occ_plan_clear()
        i = ctx.occ_lattice_info()
        assert (i.built, i.stale) == (1, 1) and build() == LV_ESTATE and ctx.occ_lattice_info().built == 1
        # (that lattice was built on TABLE1's plan; back to the first one, then the grid moves under the snapshot)
        ctx.occ_distance_build(capi.default_distance_params(**DP))
        ctx.occ_plan_build(goal3, TABLE6, capi.default_plan_params(connectivity=8))
        assert build() == 0 and same()
        ctx.volume_recentre(capi.LV_VOLUME_OCC, (3, -2, 0))
        assert same() and ctx.occ_lattice_info().stale == 0
        # lv_occ_lattice_clear discards it; so does lv_occ_configure
        ctx.occ_lattice_clear()
        assert ctx.occ_lattice_info().built == 0 and fetch_and_paths() == (LV_ESTATE, LV_ESTATE)
        ctx.occ_distance_build(capi.default_distance_params(**DP))
        ctx.occ_plan_build(goal3, TABLE6, capi.default_plan_params(connectivity=8))
        assert build() == 0 and ctx.occ_lattice_info().built == 1
        ctx.occ_configure(capi.default_occupancy_params(**dict(prm, nx=44)))
        assert ctx.occ_lattice_info().built == 0 and fetch_and_paths() == (LV_ESTATE, LV_ESTATE)


# ---- 8. the generator's tables through plan / routes
@pytest.mark.parametrize("radius,reverse", [(0.5, False), (1.0, False), (1.0, True)])
def test_generated_primitives_route_to_a_goal_behind(capi, radius, reverse):
    from limo_velo_amd import lattice

    nx, ny, H = 45, 37, 16
    prm = _params(nx, ny)
    rng = np.random.default_rng(3)
    mask = rng.uniform(size=(ny, nx)) < 0.02
    mask[14:23, 10:36] = False
    t = lattice.primitives(H, radius, prm["resolution"], reverse=reverse, reverse_penalty=300, turn_penalty=2)
    assert t.shape == (H, 6 if reverse else 3) and lr.check_table(H, t.shape[1], t) is None
    lattice.check_primitives(t)
    th = lattice.headings(H)
    assert lattice.heading_index(th[5] + 0.01, H) == 5 and np.allclose(np.tan(th[1]), 0.5)
    start = _centre(prm, 26, 18, 0)
    goal = _centre(prm, 18, 18, 0)   # directly behind a car that faces +x
    with capi.Context() as ctx:
        c = _plan(capi, ctx, prm, mask)
        info, st = lattice.plan(ctx, [[goal[0], goal[1], 0.0]], t)
        goals = lr.poses([goal])
        rV, rst = lr.build(prm, c, t, goals)
        assert np.array_equal(ctx.occ_lattice_fetch(), rV) and list(st) == list(rst) and (info.built, info.H, info.P) == (1, H, t.shape[1])
        (poses, taken, status, cost), = lattice.routes(ctx, [[start[0], start[1], 0.0]])
        rstatus, rcost, roff, rstates, rtaken = lr.paths(prm, c, rV, t, lr.poses([start]))
        assert status == rstatus[0] == 0 and cost == rcost[0] and np.array_equal(taken, rtaken)
        hs = rstates.astype(np.int64) // (nx * ny)
        cells = rstates.astype(np.int64) % (nx * ny)
        assert np.array_equal(poses[:, 2], th[hs])
        assert np.array_equal(poses[:, :2], np.stack([prm["origin"][0] + (cells % nx + 0.5) * 0.25, prm["origin"][1] + (cells // nx + 0.5) * 0.25], axis=1))
        step = np.abs((np.diff(hs) + H // 2) % H - H // 2)
        assert np.all(step <= 1)   # (every primitive of the generator keeps the heading or moves it one bin, driven either way)
        if not reverse:   # forward only, it has to turn right round: through every bin on one side, one bin a step
            assert {0, 8} <= set(hs.tolist()) and (4 in hs or 12 in hs) and np.all(taken[:-1] < 3)
        line = lattice.polyline((poses, taken, status, cost), t)
        assert len(line) >= len(poses) and np.array_equal(line[0], poses[0, :2]) and np.array_equal(line[-1], poses[-1, :2])
