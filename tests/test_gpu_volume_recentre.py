"""GPU tests of the rolling volumes (lv_volume_recentre, lv_volume_shift_info, lv_occ_mark; include/limovelo_hip.h "Rolling
volumes") against the numpy statement of the rule in tests/recentre_ref.py.  Contents move by whole voxels and the origin is two
f32 operations, so every comparison is by equality of bits: log-odds as uint32 (a NaN's payload included), S and W as integers,
origins as bits, stats as integers.

The no-op case holds what a caller can see of "d = 0 touches nothing" (the bits, the stale flags, the shifts, the stats), and that
it does not allocate the grid's second buffer: the device's free memory (hipMemGetInfo) before and after, on a grid whose buffer
is 32 MiB, with the first non-zero shift as the control that the measure sees that buffer."""
import ctypes as C

import numpy as np
import pytest

import occupancy_ref as ocr
import recentre_ref as rr
import rollout_cases as cases
import tsdf_cases as tc
import tsdf_ref as tr

pytestmark = pytest.mark.gpu

LV_OK, LV_EINVAL, LV_ESTATE = 0, -1, -4
F = np.float32
ORIGIN0, RES = (-1.0, -0.5, -0.25), 0.25


@pytest.fixture(scope="module")
def capi(lv):
    from limo_velo_amd import capi as c

    return c


@pytest.fixture(scope="module")
def ctx(capi):
    """One context for the module: every test configures the volumes it needs."""
    with capi.Context() as c:
        yield c


def _occ_prm(dims, origin=ORIGIN0):
    return ocr.params(origin=tuple(float(v) for v in origin), resolution=RES, nx=dims[0], ny=dims[1], nz=dims[2], min_range=0.3, max_range=6.0)


def _tsdf_prm(dims, origin=ORIGIN0, **kw):
    return tr.params(origin=tuple(float(v) for v in origin), resolution=RES, nx=dims[0], ny=dims[1], nz=dims[2], min_range=0.3, max_range=6.0, **kw)


def _centre(dims, origin=ORIGIN0):
    return tuple(float(origin[a]) + 0.5 * dims[a] * RES + 0.07 for a in range(3))


def _sweeps(dims, seed, n=2, origin=ORIGIN0):
    rng = np.random.default_rng(seed)
    c = np.array(_centre(dims, origin))
    return [tc.random_view(rng, c + rng.uniform(-0.3, 0.3, 3), n=600) for _ in range(n)]


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _origin_bits(p):
    return [int(v) for v in np.array([v for v in p.origin], F).view(np.uint32)]


def _recentre_raw(capi, ctx, volume, d, stats=None):
    return ctx.lib.lv_volume_recentre(ctx.h, volume, (C.c_int32 * 3)(*[int(v) for v in d]), stats)


# ---- 1. a shift equals the slice assignment
@pytest.mark.parametrize("dims", [(33, 5, 3), (70, 37, 9)] + rr.ALIGNED_GRIDS)
def test_occupancy_shift_equals_the_reference(capi, ctx, dims):
    """nx = 33 and 70: row tails and unaligned sources, every shift through the dword-load kernel.  nx = 36 and 72: the shifts with
    d_x % 4 == 0 run the 16-byte-load kernel (the one the default 512-wide grid and steps of 32 take), the others the dword one."""
    prm = _occ_prm(dims)
    ctx.occ_configure(capi.default_occupancy_params(**prm))
    ctx.occ_integrate(_sweeps(dims, 1))
    L0 = ctx.occ_fetch()
    L0.reshape(-1).view(np.uint32)[-1] = 0x7FC00001   # a NaN with another payload: no evidence, and its bits must survive
    evidence = ~np.isnan(L0)
    assert evidence.sum() > 50 and (~evidence).sum() > 50
    s = np.zeros(3, np.int64)
    shifts = rr.shift_list(dims)
    aligned = [d for d in shifts if dims[0] % 4 == 0 and d[0] % 4 == 0 and any(d)]   # the shifts that take the 16-byte-load kernel
    if dims[0] % 4 == 0:
        assert sum(1 for d in aligned if 0 < abs(d[0]) < dims[0] and d[1] and d[2]) >= 6 and any(d[0] == 0 and d[1] for d in aligned)
        assert any(abs(d[0]) >= dims[0] for d in aligned) and any(d[0] % 4 for d in shifts)
        assert any(rr.stats(evidence, d)[2] > 0 and 0 < rr.stats(evidence, d)[0] for d in aligned)   # some evidence leaves, some stays
    else:
        assert not aligned and any(d[0] % 4 == 0 and d[0] for d in shifts)
    for d in shifts:
        ctx.occ_load(L0)   # (the contents start over; the accumulated shift goes on)
        st = ctx.volume_recentre(capi.LV_VOLUME_OCC, d)
        s += np.array(d)
        want = rr.shifted(_bits(L0), d, rr.NAN_BITS)
        assert np.array_equal(_bits(ctx.occ_fetch()), want), d
        assert [int(v) for v in st] == (rr.stats(evidence, d) if any(d) else [0, 0, 0, 0]), d   # (a zero shift does nothing and counts nothing)
        p = ctx.occ_params()
        assert _origin_bits(p) == [int(v) for v in rr.origin_at(ORIGIN0, s, RES).view(np.uint32)], (d, s)
        assert (p.nx, p.ny, p.nz, p.resolution) == (dims[0], dims[1], dims[2], F(RES))
        assert list(ctx.volume_shift_info().grid) == list(s)
        if any(abs(d[a]) >= dims[a] for a in range(3)):   # everything leaves
            assert np.all(want == rr.NAN_BITS) and int(st[2]) == int(evidence.sum()) and int(st[0]) == 0
    # ... and home again: the origin is origin0, bit for bit
    ctx.volume_recentre(capi.LV_VOLUME_OCC, -s)
    assert _origin_bits(ctx.occ_params()) == [int(v) for v in np.asarray(ORIGIN0, F).view(np.uint32)]
    assert not any(ctx.volume_shift_info().grid)


@pytest.mark.parametrize("dims", [(33, 5, 3), (70, 37, 9)])
def test_tsdf_shift_equals_the_reference_and_leaves_the_scratch_zero(capi, ctx, dims):
    prm = _tsdf_prm(dims, carve=1)
    ctx.tsdf_configure(capi.default_tsdf_params(**prm))
    ctx.tsdf_integrate(_sweeps(dims, 2))
    v0 = ctx.tsdf_fetch()
    S0, W0 = v0["S"], v0["W"]
    assert (W0 > 0).sum() > 50 and (W0 == 0).sum() > 50
    s = np.zeros(3, np.int64)
    for d in rr.shift_list(dims):
        ctx.tsdf_load(S0, W0)
        st = ctx.volume_recentre(capi.LV_VOLUME_SURFACE, d)
        s += np.array(d)
        got = ctx.tsdf_fetch()
        assert np.array_equal(got["S"], rr.shifted(S0, d, 0)) and np.array_equal(got["W"], rr.shifted(W0, d, 0)), d
        assert [int(v) for v in st] == (rr.stats(W0 > 0, d) if any(d) else [0, 0, 0, 0]), d
        assert _origin_bits(ctx.tsdf_params()) == [int(v) for v in rr.origin_at(ORIGIN0, s, RES).view(np.uint32)], (d, s)
        assert list(ctx.volume_shift_info().surface) == list(s)
    ctx.volume_recentre(capi.LV_VOLUME_SURFACE, -s)
    assert _origin_bits(ctx.tsdf_params()) == [int(v) for v in np.asarray(ORIGIN0, F).view(np.uint32)]
    # the scratch staged every one of those moves: a fusion on top must find it all zero
    d = (3, -2, 1)
    ctx.tsdf_load(S0, W0)
    ctx.volume_recentre(capi.LV_VOLUME_SURFACE, d)
    origin = rr.origin_at(ORIGIN0, d, RES)
    view = _sweeps(dims, 3, n=1, origin=origin)
    S, W, rst = tr.integrate(_tsdf_prm(dims, origin, carve=1), rr.shifted(S0, d, 0), rr.shifted(W0, d, 0), view)
    assert list(ctx.tsdf_integrate(view)) == list(rst)
    got = ctx.tsdf_fetch()
    assert np.array_equal(got["S"], S) and np.array_equal(got["W"], W)


# ---- 2. recentre equals reconfigure at the new origin
def _rays(dims, origin, rng, n=64):
    lo = np.asarray(origin, np.float64)
    hi = lo + RES * np.array(dims)
    return rng.uniform(lo - 0.5, hi + 0.5, (n, 3)).astype(F), rng.uniform(lo - 0.5, hi + 0.5, (n, 3)).astype(F)


def test_occupancy_recentre_equals_reconfigure(capi, ctx):
    dims, d = (70, 37, 9), (5, -3, 1)
    first, more = _sweeps(dims, 4), _sweeps(dims, 5)
    pattern = tc.random_view(np.random.default_rng(6), (0, 0, 0), n=600)[2]
    ctx.occ_configure(capi.default_occupancy_params(**_occ_prm(dims)))
    ctx.occ_integrate(first)
    frm, to = _rays(dims, ORIGIN0, np.random.default_rng(7))
    ctx.occ_raycast(frm, to)   # (the packed ray states exist and show the grid before the shift)
    L_before = ctx.occ_fetch()
    ctx.volume_recentre(capi.LV_VOLUME_OCC, d)
    pa = ctx.occ_params()
    origin = [float(v) for v in pa.origin]
    stats_a = ctx.occ_integrate(more)
    gain_views = [(v[0], v[1], pattern) for v in more]
    a = dict(L=ctx.occ_fetch(), proj=ctx.occ_project(0, dims[2] - 1), rays=ctx.occ_raycast(frm, to), gain=ctx.occ_view_gain(gain_views))
    with capi.Context() as b:
        b.occ_configure(capi.default_occupancy_params(**_occ_prm(dims, origin)))
        assert _origin_bits(b.occ_params()) == _origin_bits(pa)
        b.occ_load(rr.shift_logodds(L_before, d))
        assert list(b.occ_integrate(more)) == list(stats_a)
        assert np.array_equal(_bits(b.occ_fetch()), _bits(a["L"]))
        assert np.array_equal(b.occ_project(0, dims[2] - 1), a["proj"])
        assert b.occ_raycast(frm, to).tobytes() == a["rays"].tobytes()
        assert np.array_equal(b.occ_view_gain(gain_views), a["gain"])
    assert (a["rays"]["status"] == capi.LV_RAY_STOPPED).any() and a["gain"].any()


def test_tsdf_recentre_equals_reconfigure(capi, ctx):
    dims, d = (70, 37, 9), (-4, 2, -1)
    first = _sweeps(dims, 8) + [tc.wall_view(tc.INSIDE)]
    ctx.tsdf_configure(capi.default_tsdf_params(**_tsdf_prm(dims)))
    ctx.tsdf_integrate(first)
    ctx.tsdf_mesh_build(1)
    before = ctx.tsdf_fetch()
    ctx.volume_recentre(capi.LV_VOLUME_SURFACE, d)
    info = ctx.tsdf_mesh_info()
    assert info.built == 1 and info.stale == 1   # (a snapshot in metres: it stays, and says it is old)
    pa = ctx.tsdf_params()
    origin = [float(v) for v in pa.origin]
    more = _sweeps(dims, 9, origin=origin) + [tc.wall_view(tc.INSIDE)]
    stats_a = ctx.tsdf_integrate(more)
    counts_a = ctx.tsdf_mesh_build(1)
    vol_a, mesh_a = ctx.tsdf_fetch(), ctx.tsdf_mesh_fetch()
    with capi.Context() as b:
        b.tsdf_configure(capi.default_tsdf_params(**_tsdf_prm(dims, origin)))
        assert _origin_bits(b.tsdf_params()) == _origin_bits(pa)
        b.tsdf_load(rr.shifted(before["S"], d, 0), rr.shifted(before["W"], d, 0))
        assert list(b.tsdf_integrate(more)) == list(stats_a)
        vol_b = b.tsdf_fetch()
        assert np.array_equal(vol_b["S"], vol_a["S"]) and np.array_equal(vol_b["W"], vol_a["W"])
        assert list(b.tsdf_mesh_build(1)) == list(counts_a)
        mesh_b = b.tsdf_mesh_fetch()
        for k in ("sub", "tri"):
            assert np.array_equal(mesh_b[k], mesh_a[k]), k
        assert np.array_equal(_bits(mesh_b["xyz"]), _bits(mesh_a["xyz"]))
    assert int(counts_a[0]) > 0


# ---- 3. the snapshots across a shift
def _snapshot_world(capi, c, L, prm):
    c.occ_configure(capi.default_occupancy_params(**prm))
    c.occ_load(L)


def _build_snapshots(capi, c):
    c.occ_distance_build(capi.default_distance_params(**cases.DP))
    c.occ_plan_build(cases.GOAL, cases.TABLE, capi.default_plan_params(**cases.PP))
    c.occ_frontier_build(capi.default_frontier_params(planar=1, k_lo=0, k_hi=2, connectivity=8))


def _rank_raw(c):
    n = max(int(c.occ_frontier_info().n_clusters), 1)
    bp = np.full(n, 7, np.uint32)
    return c.lib.lv_occ_frontier_rank(c.h, 2, bp.ctypes.data_as(C.POINTER(C.c_uint32)), None, n)


def test_snapshots_answer_the_same_across_a_shift(capi, ctx):
    L = cases.grid()
    L[:, 3:9, 3:12] = np.nan   # an unknown patch left of the wall: frontiers
    _snapshot_world(capi, ctx, L, cases.PRM)
    _build_snapshots(capi, ctx)
    assert ctx.occ_frontier_info().n_clusters > 0 and _rank_raw(ctx) == LV_OK
    rng = np.random.default_rng(12)
    lo = np.array(cases.PRM["origin"])
    pts = rng.uniform(lo - 0.5, lo + 0.25 * np.array([cases.NX, cases.NY, cases.NZ]) + 0.5, (300, 3)).astype(F)
    b = cases.batches()["random_K65_T64_Tc1_fp5"]

    def answers():
        dist, grad = ctx.occ_distance_query(pts)
        paths = ctx.occ_plan_paths(pts[:64])
        roll = ctx.occ_rollout(b["start"], b["controls"], capi.default_rollout_params(**b["rp"]), b["fp"], ("results", "poses", "score", "best"))
        return [_bits(dist), _bits(grad)] + [np.asarray(v) for v in paths] + [roll[k] for k in ("results", "poses", "score", "best")]

    before = answers()
    d = (3, -2, 0)
    ctx.volume_recentre(capi.LV_VOLUME_OCC, d)
    assert ctx.occ_distance_info().stale == 1 and ctx.occ_frontier_info().stale == 1
    sh = ctx.volume_shift_info()
    assert list(sh.grid) == list(d) and not any(sh.field) and not any(sh.plan) and not any(sh.frontier)
    for x, y in zip(before, answers()):   # the same world points and starts: the same bits
        assert x.tobytes() == y.tobytes()
    # the frontier's cells and the plan's are of the old box: no ranking until all three are rebuilt
    assert _rank_raw(ctx) == LV_ESTATE and "shift" in ctx.lib.lv_last_error().decode()
    ctx.occ_distance_build(capi.default_distance_params(**cases.DP))
    assert list(ctx.volume_shift_info().field) == list(d) and _rank_raw(ctx) == LV_ESTATE
    ctx.occ_plan_build(cases.GOAL, cases.TABLE, capi.default_plan_params(**cases.PP))
    assert list(ctx.volume_shift_info().plan) == list(d) and _rank_raw(ctx) == LV_ESTATE
    ctx.occ_frontier_build(capi.default_frontier_params(planar=1, k_lo=0, k_hi=2, connectivity=8))
    sh = ctx.volume_shift_info()
    assert list(sh.frontier) == list(d) and _rank_raw(ctx) == LV_OK
    assert ctx.occ_distance_info().stale == 0 and ctx.occ_frontier_info().stale == 0
    # what was rebuilt is what a context configured there builds
    origin = [float(v) for v in ctx.occ_params().origin]
    with capi.Context() as fresh:
        _snapshot_world(capi, fresh, rr.shift_logodds(L, d), dict(cases.PRM, origin=tuple(origin)))
        _build_snapshots(capi, fresh)
        assert np.array_equal(fresh.occ_distance_fetch(metres=False)[0], ctx.occ_distance_fetch(metres=False)[0])
        for x, y in zip(fresh.occ_plan_fetch(), ctx.occ_plan_fetch()):
            assert np.array_equal(x, y)
        assert np.array_equal(fresh.occ_frontier_fetch(), ctx.occ_frontier_fetch())
        assert not any(fresh.volume_shift_info().grid)


# ---- 4. a shift by nothing, the refusals, the states
def test_a_zero_shift_touches_nothing_and_refusals_change_nothing(capi, ctx):
    with capi.Context() as c:   # (no volume yet)
        assert _recentre_raw(capi, c, capi.LV_VOLUME_OCC, (1, 0, 0)) == LV_ESTATE
        assert _recentre_raw(capi, c, capi.LV_VOLUME_SURFACE, (0, 0, 0)) == LV_ESTATE
        assert c.lib.lv_occ_mark(c.h, C.byref(capi.default_occ_mark_params()), None, 0, 0, None) == LV_ESTATE
        sh = c.volume_shift_info()
        assert not any(list(sh.grid) + list(sh.surface) + list(sh.field) + list(sh.plan) + list(sh.frontier))
        c.tsdf_configure(capi.default_tsdf_params(**_tsdf_prm((33, 5, 3))))
        assert _recentre_raw(capi, c, capi.LV_VOLUME_OCC, (1, 0, 0)) == LV_ESTATE    # (the other volume is)
        assert _recentre_raw(capi, c, capi.LV_VOLUME_SURFACE, (1, 0, 0)) == LV_OK
    L = cases.grid()
    L[:, 3:9, 3:12] = np.nan
    _snapshot_world(capi, ctx, L, cases.PRM)
    _build_snapshots(capi, ctx)
    ctx.tsdf_configure(capi.default_tsdf_params(**_tsdf_prm((33, 5, 3))))
    ctx.tsdf_integrate(_sweeps((33, 5, 3), 13) + [tc.wall_view(_centre((33, 5, 3)))])
    ctx.tsdf_mesh_build(1)
    vol = ctx.tsdf_fetch()
    st = np.full(4, 9, np.uint64)
    ptr = st.ctypes.data_as(C.POINTER(C.c_uint64))
    for volume in (capi.LV_VOLUME_OCC, capi.LV_VOLUME_SURFACE):
        st[:] = 9
        assert _recentre_raw(capi, ctx, volume, (0, 0, 0), ptr) == LV_OK and not st.any()
    assert np.array_equal(_bits(ctx.occ_fetch()), _bits(L))
    got = ctx.tsdf_fetch()
    assert np.array_equal(got["S"], vol["S"]) and np.array_equal(got["W"], vol["W"])
    assert ctx.occ_distance_info().stale == 0 and ctx.occ_frontier_info().stale == 0 and ctx.occ_plan_info().stale == 0
    assert ctx.tsdf_mesh_info().stale == 0 and _rank_raw(ctx) == LV_OK
    assert _origin_bits(ctx.occ_params()) == [int(v) for v in np.asarray(cases.PRM["origin"], F).view(np.uint32)]
    # the accumulated limit: up to 2^20 and no further; a refused call leaves the state as it was
    lim = 1 << 20
    ctx.volume_recentre(capi.LV_VOLUME_OCC, (lim - 3, 0, -lim))
    p = ctx.occ_params()
    for d in ((4, 0, 0), (0, 0, -1), (3, 0, -1)):
        st[:] = 9
        assert _recentre_raw(capi, ctx, capi.LV_VOLUME_OCC, d, ptr) == LV_EINVAL and "accumulated" in ctx.lib.lv_last_error().decode()
        assert list(st) == [9] * 4 and list(ctx.volume_shift_info().grid) == [lim - 3, 0, -lim] and _origin_bits(ctx.occ_params()) == _origin_bits(p)
    ctx.volume_recentre(capi.LV_VOLUME_OCC, (3, 0, 0))
    assert list(ctx.volume_shift_info().grid) == [lim, 0, -lim]
    assert np.all(_bits(ctx.occ_fetch()) == rr.NAN_BITS)
    ctx.volume_recentre(capi.LV_VOLUME_OCC, (-lim, 0, lim))
    assert _origin_bits(ctx.occ_params()) == [int(v) for v in np.asarray(cases.PRM["origin"], F).view(np.uint32)]


def _free_bytes():
    hip = C.CDLL("libamdhip64.so")
    free, total = C.c_size_t(), C.c_size_t()
    assert hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return int(free.value)


def test_a_zero_shift_does_not_allocate_the_second_buffer(capi):
    dims = (512, 256, 64)
    size = 4 * dims[0] * dims[1] * dims[2]   # 32 MiB: far above the allocator's granularity and anything else these calls need
    with capi.Context() as c:
        c.occ_configure(capi.default_occupancy_params(nx=dims[0], ny=dims[1], nz=dims[2]))
        c.volume_recentre(capi.LV_VOLUME_OCC, (0, 0, 0))   # (whatever a first call of the entry point sets up is set up)
        before = _free_bytes()
        for _ in range(3):
            assert not c.volume_recentre(capi.LV_VOLUME_OCC, (0, 0, 0)).any()
        after_zero = _free_bytes()
        assert before - after_zero < size // 2, (before, after_zero)
        c.volume_recentre(capi.LV_VOLUME_OCC, (4, 0, 0))
        after_shift = _free_bytes()
        assert after_zero - after_shift >= size // 2, (after_zero, after_shift)   # the control: the first shift allocates it ...
        c.volume_recentre(capi.LV_VOLUME_OCC, (-4, 1, 0))
        assert abs(after_shift - _free_bytes()) < size // 2                       # ... and it is kept: the next one allocates nothing
        c.occ_configure(capi.default_occupancy_params(nx=dims[0], ny=dims[1], nz=dims[2]))
        assert _free_bytes() - after_shift >= size // 2                           # configure frees it


# ---- 5. marking voxels from points
MARK_DIMS = (33, 5, 3)


def _voxel_points(origin, cells, counts, rng):
    """counts[i] points inside voxel cells[i], away from its faces."""
    out = []
    for (i, j, k), c in zip(cells, counts):
        lo = np.array(origin, np.float64) + RES * np.array([i, j, k])
        out.append(lo + RES * rng.uniform(0.1, 0.9, (c, 3)))
    return np.concatenate(out).astype(F)


def _mark_case():
    rng = np.random.default_rng(21)
    L = np.full(MARK_DIMS[::-1], np.nan, F)
    L[1, 2, 5] = -0.4      # observed free
    L[1, 2, 6] = 3.4       # observed, close to l_max
    L[0, 1, 20] = -1.9     # observed, close to l_min
    cells = [(4, 2, 1), (5, 2, 1), (6, 2, 1), (7, 2, 1), (20, 1, 0), (32, 4, 2), (0, 0, 0), (12, 3, 2)]
    counts = [3, 3, 4, 2, 3, 3, 5, 1]      # min_points 3: (7, 2, 1) misses it by one, (4, 2, 1) hits it exactly
    pts = _voxel_points(ORIGIN0, cells, counts, rng)
    o = np.array(ORIGIN0, F)
    far = (o + F(RES) * np.array(MARK_DIMS, F)).astype(F)
    extra = np.array([o, o, o,                                                # on the low faces: voxel (0, 0, 0)
                      [far[0], o[1], o[2]], [o[0], far[1], o[2]], far,      # on the far faces: outside
                      [-50.0, 0.0, 0.0], [0.0, 0.0, 9.0], [1e30, 0.0, 0.0],  # outside the grid
                      [np.nan, 0.0, 0.0], [0.0, np.inf, 0.0], [0.0, 0.0, -np.inf]], F)
    pts = np.concatenate([pts, extra]).astype(F)
    return L, pts[rng.permutation(len(pts))]


@pytest.mark.parametrize("only_unknown", [1, 0])
@pytest.mark.parametrize("l_mark", [0.85, -0.4])
def test_mark_from_caller_points(capi, ctx, only_unknown, l_mark):
    L, pts = _mark_case()
    prm = _occ_prm(MARK_DIMS)
    whole = ((0, 0, 0), (2 ** 30, 2 ** 30, 2 ** 30))
    boxes = [whole, ((4, 0, 0), (6, 4, 2)), ((-9, -9, -9), (5, 2, 1)), ((40, 0, 0), (50, 4, 2)), ((0, 0, 3), (32, 4, 9)), ((5, 3, 0), (4, 4, 2))]
    ctx.occ_configure(capi.default_occupancy_params(**prm))
    for lo, hi in boxes:
        want, rst = rr.mark(prm, L, pts, lo, hi, 3, only_unknown, l_mark)
        for order in (pts, pts[::-1].copy()):   # a pure function of the point set
            ctx.occ_load(L)
            ctx.occ_distance_build(capi.default_distance_params())
            st = ctx.occ_mark(capi.default_occ_mark_params(lo=lo, hi=hi, min_points=3, only_unknown=only_unknown, l_mark=l_mark), order)
            assert [int(v) for v in st] == rst, (lo, hi)
            assert np.array_equal(_bits(ctx.occ_fetch()), _bits(want)), (lo, hi)
            assert ctx.occ_distance_info().stale == (1 if rst[2] else 0)   # (stale iff a voxel was written)
        if rr.clip_box(MARK_DIMS, lo, hi) is None:
            assert rst == [0, 0, 0, 0]
    want, rst = rr.mark(prm, L, pts, *whole, 3, only_unknown, l_mark)
    assert rst[1] == 6 and rst[0] == 3 + 3 + 4 + 2 + 3 + 3 + 5 + 1 + 3
    assert np.isnan(want[1, 2, 7]) and np.isnan(want[2, 3, 12])          # one point short, and a single point
    if only_unknown:
        assert rst[2] == 3 and rst[3] == 3
        assert _bits(want)[1, 2, 5] == _bits(L)[1, 2, 5] and _bits(want)[1, 2, 6] == _bits(L)[1, 2, 6]   # observed: left alone
        assert want[1, 2, 4] == F(l_mark)
    else:
        assert rst[2] == 6 and rst[3] == 0
        assert want[1, 2, 5] == F(F(-0.4) + F(l_mark)) and want[1, 2, 6] == (F(3.5) if l_mark > 0 else F(F(3.4) + F(l_mark)))
        assert want[0, 1, 20] == (F(-2.0) if l_mark < 0 else F(F(-1.9) + F(l_mark)))                      # moved by l_mark, clamped
    # min_points 1 and a grid that has been shifted: the points are placed by the origin of now
    d = (2, -1, 0)
    ctx.occ_load(L)
    ctx.volume_recentre(capi.LV_VOLUME_OCC, d)
    prm2 = _occ_prm(MARK_DIMS, rr.origin_at(ORIGIN0, d, RES))
    want, rst = rr.mark(prm2, rr.shift_logodds(L, d), pts, *whole, 1, only_unknown, l_mark)
    st = ctx.occ_mark(capi.default_occ_mark_params(min_points=1, only_unknown=only_unknown, l_mark=l_mark), pts)
    assert [int(v) for v in st] == rst and np.array_equal(_bits(ctx.occ_fetch()), _bits(want))


def test_mark_from_the_map_equals_mark_from_its_points(capi, ctx):
    rng = np.random.default_rng(31)
    prm = _occ_prm(MARK_DIMS)
    lo = np.array(ORIGIN0)
    hi = lo + RES * np.array(MARK_DIMS)
    cloud = rng.uniform(lo - 0.5, hi + 0.5, (4000, 3)).astype(F)
    L, _ = _mark_case()
    ctx.occ_configure(capi.default_occupancy_params(**prm))
    st0 = ctx.occ_mark(None, None)   # (no map: no points, nothing marked)
    assert not st0.any() and np.all(_bits(ctx.occ_fetch()) == rr.NAN_BITS)
    ctx.map_build(cloud)
    gone = ctx.map_evict_box((2.0, -9.0, -9.0), (4.0, 9.0, 9.0), keep_inside=False)   # a slab of the map goes
    living = ctx.map_fetch()
    assert gone > 100 and 100 < len(living) < len(cloud)
    for only_unknown, min_points in ((1, 1), (1, 2), (0, 2)):
        p = capi.default_occ_mark_params(min_points=min_points, only_unknown=only_unknown, lo=(1, 0, 0), hi=(30, 4, 2))
        ctx.occ_load(L)
        st_map = ctx.occ_mark(p, None)
        from_map = ctx.occ_fetch()
        ctx.occ_load(L)
        st_pts = ctx.occ_mark(p, living)
        assert list(st_map) == list(st_pts) and np.array_equal(_bits(from_map), _bits(ctx.occ_fetch()))
        want, rst = rr.mark(prm, L, living, (1, 0, 0), (30, 4, 2), min_points, only_unknown, 0.85)
        assert [int(v) for v in st_map] == rst and np.array_equal(_bits(from_map), _bits(want))
        slab = from_map[:, :, 13:19]   # x 2.25 .. 3.75 m: inside the evicted slab, no living point
        assert np.array_equal(_bits(slab), _bits(L[:, :, 13:19])) and int(st_map[2]) > 20


# ---- 6. Python: follow, exposed_boxes, mark_from_map, explore
def test_follow_a_drive_and_fill_the_strips_from_the_map(capi, ctx):
    from limo_velo_amd import mesh, occupancy

    dims, res, keep, step = (128, 96, 8), 0.2, 0.25, 16
    origin0 = (-12.8, -9.6, -0.8)
    prm = ocr.params(origin=origin0, resolution=res, nx=dims[0], ny=dims[1], nz=dims[2], min_range=0.3, max_range=20.0)
    ctx.occ_configure(capi.default_occupancy_params(**prm))
    ctx.tsdf_configure(mesh.like_occupancy(ctx.occ_params()))
    rng = np.random.default_rng(41)
    # the map: points along the whole drive, in the grid's height
    cloud = np.stack([rng.uniform(-15, 215, 60000), rng.uniform(-12, 112, 60000), rng.uniform(-0.7, 0.7, 60000)], axis=1).astype(F)
    ctx.map_build(cloud)
    free = np.full(dims[::-1], -1.0, F)
    total = np.zeros(3, np.int64)
    moved = 0
    for x in np.arange(0.0, 200.0 + 1e-9, 5.0):
        pos = (x, 0.5 * x, 0.0)
        ctx.occ_load(free)   # everything observed: whatever is unknown afterwards was exposed by this step
        d = occupancy.follow(ctx, pos, keep=keep, step=step)
        assert mesh.follow(ctx, pos, keep=keep, step=step) == d and d[2] == 0
        total += np.array(d)
        p = ctx.occ_params()
        assert list(ctx.volume_shift_info().grid) == list(total) == list(ctx.volume_shift_info().surface)
        assert _origin_bits(p) == _origin_bits(ctx.tsdf_params())
        vox = np.floor((np.array(pos, F) - np.array([v for v in p.origin], F)) / F(res))
        for a in range(2):
            assert abs(int(vox[a]) - dims[a] // 2) <= keep * dims[a] + step, (pos, d)
            assert d[a] % step == 0
        Lf = ctx.occ_fetch()
        unknown = np.isnan(Lf)
        boxes = occupancy.exposed_boxes(p, d)
        cover = np.zeros(unknown.shape, np.int32)
        for lo, hi in boxes:
            cover[lo[2]:hi[2] + 1, lo[1]:hi[1] + 1, lo[0]:hi[0] + 1] += 1
        assert cover.max() <= 1 and np.array_equal(cover == 1, unknown) and len(boxes) <= 3   # disjoint, and exactly the exposed voxels
        if not any(d):
            assert not boxes
            continue
        moved += 1
        marked = sum((occupancy.mark_from_map(ctx, box) for box in boxes), np.zeros(4, np.uint64))
        Lm = ctx.occ_fetch()
        assert np.array_equal(_bits(Lm)[~unknown], _bits(Lf)[~unknown])            # only the strips were filled
        want, rst = rr.mark(ocr.params_of(p), Lf, ctx.map_fetch(), (0, 0, 0), tuple(v - 1 for v in dims), 1, 1, 0.85)
        assert np.array_equal(_bits(Lm), _bits(want)) and int(marked[2]) == rst[2] > 0
    assert moved >= 5 and total[0] > 800 and total[1] > 400
    # exploring from the last pose after one more step of the grid: the strip it exposed is unknown next to free space
    ctx.occ_load(free)
    occupancy.recentre(ctx, (step, 0, 0))
    total[0] += step
    cl, lines = occupancy.explore(ctx, pos, 0.3, z_band=(-0.5, 0.5), unknown="free")
    assert len(cl) > 0 and (cl["best_cell"] >= 0).any() and any(len(ln) for ln in lines)
    sh = ctx.volume_shift_info()
    assert list(sh.field) == list(sh.plan) == list(sh.frontier) == list(total)


def test_a_saved_recentred_volume_loads_where_it_was(capi, ctx, tmp_path):
    from limo_velo_amd import mesh, occupancy

    dims, d = (33, 5, 3), (7, -1, 1)
    ctx.occ_configure(capi.default_occupancy_params(**_occ_prm(dims)))
    ctx.occ_integrate(_sweeps(dims, 51))
    ctx.tsdf_configure(capi.default_tsdf_params(**_tsdf_prm(dims)))
    ctx.tsdf_integrate(_sweeps(dims, 52))
    occupancy.recentre(ctx, d)
    mesh.recentre(ctx, d)
    La, va = ctx.occ_fetch(), ctx.tsdf_fetch()
    occupancy.save_grid(ctx, str(tmp_path / "grid.npz"))
    mesh.save(ctx, str(tmp_path / "vol"))
    with capi.Context() as b:
        p = occupancy.load_grid(b, str(tmp_path / "grid.npz"))
        q = mesh.load(b, str(tmp_path / "vol"))
        want = [int(v) for v in rr.origin_at(ORIGIN0, d, RES).view(np.uint32)]
        assert _origin_bits(b.occ_params()) == _origin_bits(p) == want == _origin_bits(q) == _origin_bits(b.tsdf_params())
        assert np.array_equal(_bits(b.occ_fetch()), _bits(La))
        vb = b.tsdf_fetch()
        assert np.array_equal(vb["S"], va["S"]) and np.array_equal(vb["W"], va["W"])
        assert not any(b.volume_shift_info().grid)   # (configured there: its own origin0)
