"""The resident localisation filter (include/limovelo_hip.h "Resident localisation filter") on the GPU, through capi, against
tests/mcl_filter_ref.py: after every call the fetched poses (by their bits), acc, n_in, best, the statistics and the ancestors equal
the reference's, no tolerance.  The world and the fields are those of tests/mcl_cases.py (a room of 40 x 30 x 3 cells).  Sequences of
three cycles at K = 1, 2, 63, 64, 65, 255, 256, 257, 4097 and 65537 (a wavefront, a workgroup, and the first and second level of the
block sums), B = 1, 3, 64, 65, the planar and the 3-D field, weight tables of 1, 2 and 4096 entries, shift 0 and 3, modes 0, 1, 2; the
degenerate particle sets; what the calls must leave alone; the states and the limits; and the closed loop of mcl.DeviceFilter.

The tracking bound of test_closed_loop_tracking is measured, not guessed (DESIGN.md "Resident localisation filter"): the reference
filter alone, seeds 0..4, ends 0.0781, 0.0803, 0.0713, 0.0707, 0.0780 m and 0.0288, 0.0279, 0.0296, 0.0298, 0.0269 rad from the truth
(tests/test_mcl_filter_ref.py prints and bounds them); twice the worst is 0.161 m and 0.060 rad, below the floor of one cell (0.25 m)
and 10 degrees that the existing tracking test argues, so the floor is the bound."""
import ctypes as C

import numpy as np
import pytest

import mcl_cases as cases
import mcl_filter_ref as fr
import mcl_ref as mr

pytestmark = pytest.mark.gpu

LV_OK, LV_EINVAL, LV_ESTATE = 0, -1, -4
F = np.float32
NO = np.uint64(mr.NO_SCORE)
TRACK_BOUND_M, TRACK_BOUND_RAD = 0.25, float(np.radians(10.0))


@pytest.fixture(scope="module")
def capi(lv):
    from limo_velo_amd import capi as c

    return c


class World:
    """One context holding the room; use(name) builds the named field when it is not the one last built."""

    def __init__(self, capi, ctx):
        self.capi, self.ctx, self.name = capi, ctx, None
        ctx.occ_configure(capi.default_occupancy_params(**cases.PRM))
        ctx.occ_load(cases.grid())

    def use(self, name):
        if name != self.name:
            self.ctx.occ_distance_build(self.capi.default_distance_params(**cases.DPS[name]))
            assert np.array_equal(self.ctx.occ_distance_fetch(metres=False)[0], cases.field(name)["s2"])
            self.name = name
        return self.ctx


@pytest.fixture(scope="module")
def world(capi):
    with capi.Context() as c:
        yield World(capi, c)


class Pair:
    """The device's filter and the reference's, driven together: every call's outputs are compared, and check() compares what
    lv_occ_mcl_filter_get fetches."""

    def __init__(self, capi, ctx, field):
        self.capi, self.dev, self.ref = capi, ctx, fr.RefFilterContext(field)

    def set(self, poses, seed):
        self.dev.occ_mcl_filter_set(poses, seed)
        self.ref.occ_mcl_filter_set(poses, seed)
        return self.check()

    def move(self, delta, sigma):
        self.dev.occ_mcl_filter_move(delta, sigma)
        self.ref.occ_mcl_filter_move(delta, sigma)
        return self.check()

    def weigh(self, beams, table, want_best=True, **mp):
        p = mr.mparams(**mp)
        got = self.dev.occ_mcl_filter_weigh(beams, table, self.capi.default_mcl_params(**p), want_best)
        want = self.ref.occ_mcl_filter_weigh(beams, table, type("P", (), p), want_best)
        assert (got is None and want is None) or (got.dtype == np.int64 and np.array_equal(got, want)), (got, want)
        self.check()
        return want

    def resample(self, wtable, want_ancestors=True, **rp):
        got, ga = self.dev.occ_mcl_filter_resample(wtable, self.capi.default_mcl_resample_params(**rp), want_ancestors)
        want, wa = self.ref.occ_mcl_filter_resample(wtable, fr.rparams(**rp), want_ancestors)
        assert fr.stats_dict(got) == fr.stats_dict(want), (fr.stats_dict(got), fr.stats_dict(want))
        assert (ga is None) == (wa is None) and (ga is None or (ga.dtype == np.uint32 and np.array_equal(ga, wa)))
        self.check()
        return want, wa

    def check(self):
        got, want = self.dev.occ_mcl_filter_get(), self.ref.occ_mcl_filter_get()
        for k in ("poses", "acc", "n_in"):
            g, w = got[k], want[k]
            assert g.dtype == w.dtype and g.shape == w.shape, k
            if k == "poses":
                g, w = g.view(np.uint32), w.view(np.uint32)
            assert np.array_equal(g, w), (k, np.nonzero(g != w)[0][:8])
        gi, wi = self.dev.occ_mcl_filter_info(), self.ref.occ_mcl_filter_info()
        assert (gi.set, gi.K, gi.seed, gi.epoch, gi.since_resample) == (wi.set, wi.K, wi.seed, wi.epoch, wi.since_resample)
        return want


def wtable_of(n_w):
    return np.rint(1048576.0 * np.exp(-np.arange(n_w) / 40.0)).astype(np.uint32)


SEQUENCES = [(1, 3, "planar", 1, 0, 2), (2, 1, "vol", 2, 3, 1), (63, 64, "planar", 4096, 0, 1), (64, 65, "vol", 4096, 3, 2), (65, 1, "planar", 2, 0, 0),
             (255, 3, "vol", 4096, 0, 1), (256, 64, "planar", 1, 3, 2), (257, 65, "vol", 4096, 0, 1), (4097, 65, "planar", 4096, 3, 1),
             (65537, 3, "vol", 4096, 0, 2), (65537, 64, "planar", 4096, 0, 1)]


@pytest.mark.parametrize("K,B,fname,n_w,shift,mode", SEQUENCES)
def test_three_cycles_against_the_reference(capi, world, K, B, fname, n_w, shift, mode):
    b = cases.random_batch(7 * K + B, K, B, n_table=512, fname=fname)
    if K <= 2:
        b["poses"][:, :3] = [4.0, 1.0, 0.2]   # (in the room: somebody is eligible)
    mp = dict(out_cost=(0, 900)[K & 1], min_inside=min(B, K % 3))
    rng = np.random.default_rng(K)
    ctx = world.use(fname)
    pair = Pair(capi, ctx, cases.field(fname))
    pair.set(b["poses"], K + 1000)
    resampled = []
    for cycle in range(3):
        delta = np.array([rng.uniform(-0.2, 0.2), rng.uniform(0.1, 0.4), rng.uniform(-0.2, 0.2)], F)
        moved = pair.move(delta, np.array([0.05, 0.03, 0.05], F))
        before = pair.ref.acc.copy()
        pair.weigh(b["beams"], b["table"], want_best=cycle != 1, **mp)
        if cycle == 0:
            # the new path tied to the old one: lv_occ_mcl_weigh of the fetched poses gives the scores the filter accumulated
            old = ctx.occ_mcl_weigh(moved["poses"], b["beams"], b["table"], capi.default_mcl_params(**mp))
            got = ctx.occ_mcl_filter_get(("acc", "n_in"))
            assert np.array_equal(got["acc"], fr.accumulate(before, old["score"])) and np.array_equal(got["n_in"], old["n_in"])
        st, anc = pair.resample(wtable_of(n_w), want_ancestors=cycle != 2, shift=shift, mode=mode)
        resampled.append(st.resampled)
    if mode == 0:
        assert not any(resampled)
    elif K != 2:   # (two particles never have n_eff < 1 = K / 2)
        assert any(resampled)


def _degenerate():
    b = cases.random_batch(5, 12, 33, out_cost=50)
    x = b["poses"].copy()
    x[:, :2] = [4.0, 1.0]
    x[:9, 3] = [0.3, 1048576.0, -1048576.0, np.nan, np.inf, -np.inf, 1048575.9375, -1048575.9375, 2.0e6]
    x[9, :3] = [1.0e9, -3.0e38, np.nan]
    x[10, :2] = [np.inf, 5000.0]
    x[11, 3] = 3.1
    return b, x


def test_degenerate_particles(capi, world):
    """Unusable and NaN headings before and after a move, particles far outside the field (n_clamped), weighing twice without a
    move, min_inside above n_in, all weights zero, and one particle holding all the weight."""
    b, x = _degenerate()
    d, s = np.array([0.125, 0.3, 0.05], F), np.array([0.01, 0.02, 0.01], F)
    wt = np.array([1 << 20, 5, 0], np.uint32)
    pair = Pair(capi, world.use("planar"), cases.field("planar"))
    pair.set(x, 3)
    moved = pair.move(d, s)["poses"]
    assert np.array_equal(moved[[1, 2, 3, 4, 5, 8]].view(np.uint32), x[[1, 2, 3, 4, 5, 8]].view(np.uint32))   # untouched
    assert not mr.usable(moved[6, 3]) and moved[6, 0] == x[6, 0] and moved[6, 3] != x[6, 3]                   # a is unusable: x, y stay
    assert moved[11, 3] < 0                                                                                    # wrapped
    pair.weigh(b["beams"], b["table"], **b["mp"])
    once = pair.ref.acc.copy()
    pair.weigh(b["beams"], b["table"], **b["mp"])
    ok = once != NO
    assert ok.any() and np.array_equal(pair.ref.acc[ok], 2 * once[ok]) and np.all(pair.ref.acc[~ok] == NO)    # twice without a move: twice the score
    st, anc = pair.resample(wt, mode=0)
    assert st.n_clamped == 2 and st.resampled == 0 and anc is None and 0 < st.n_eligible < 12 and st.since_resample == 2
    pair.move(d, s)
    pair.weigh(b["beams"], b["table"], **b["mp"])
    st, anc = pair.resample(wt, mode=2)
    assert st.resampled == 1 and st.since_resample == 0 and not pair.ref.acc.any()
    # min_inside above every n_in: nobody is eligible, W = 0, nothing moves
    before = pair.check()["poses"].copy()
    pair.weigh(b["beams"], b["table"], min_inside=33, out_cost=1)
    assert pair.ref.n_in.max() < 33
    st, anc = pair.resample(wt, mode=2)
    assert (st.W, st.n_eligible, st.s_min, st.resampled) == (0, 0, -1, 0) and anc is None
    assert np.array_equal(pair.check()["poses"].view(np.uint32), before.view(np.uint32))
    # all weights zero with eligible particles: nothing moves either
    pair.set(x, 3)
    pair.weigh(b["beams"], b["table"], **b["mp"])
    st, anc = pair.resample(np.zeros(4, np.uint32), mode=2)
    assert st.W == 0 and st.resampled == 0 and st.s_min >= 0 and st.n_eligible > 0
    assert np.array_equal(pair.check()["poses"].view(np.uint32), x.view(np.uint32))
    # one particle holds all the weight: every ancestor is that index
    b2 = cases.random_batch(9, 300, 64)
    y = b2["poses"].copy()
    y[:, :2] += F(500.0)
    y[77] = [4.5, 2.5, 0.2, 0.25]
    pair.set(y, 1)
    pair.weigh(b2["beams"], b2["table"], **b2["mp"])
    st, anc = pair.resample(np.array([9, 1], np.uint32), mode=2)
    assert np.all(anc == 77) and (st.n_eligible, st.W, st.n_clamped) == (1, 9, 0)
    assert np.all(pair.check()["poses"].view(np.uint32) == y[77].view(np.uint32))


def test_the_same_sequence_twice_and_another_seed(capi, world):
    ctx = world.use("planar")
    b = cases.random_batch(21, 1000, 64, out_cost=200)
    table, wt = b["table"], wtable_of(4096)

    def run(seed):
        out = []
        ctx.occ_mcl_filter_set(b["poses"], seed)
        for cycle in range(3):
            ctx.occ_mcl_filter_move(np.array([0.1, 0.3, 0.05], F), np.array([0.05, 0.03, 0.05], F))
            best = ctx.occ_mcl_filter_weigh(b["beams"], table, capi.default_mcl_params(**b["mp"]))
            st, anc = ctx.occ_mcl_filter_resample(wt, capi.default_mcl_resample_params(mode=2), True)
            got = ctx.occ_mcl_filter_get()
            out.append(b"".join([best.tobytes(), bytes(st), anc.tobytes(), got["poses"].tobytes(), got["acc"].tobytes(), got["n_in"].tobytes()]))
        return out, got["poses"]

    first, p1 = run(5)
    again, _ = run(5)
    other, p2 = run(6)
    assert first == again
    assert not np.array_equal(p1, p2)


def test_nothing_else_changes_and_the_filter_outlives_the_grid(capi):
    with capi.Context() as ctx:
        w = World(capi, ctx)
        w.use("planar")
        ctx.occ_plan_build(np.array([[6.0, -1.0, 0.0]], F), np.array([250, 120, 40, 10, 3, 1], np.uint8), capi.default_plan_params(connectivity=8, min_clear_s2=2))
        ctx.occ_frontier_build(capi.default_frontier_params(planar=1, k_lo=0, k_hi=2, connectivity=8))
        b = cases.batches()["random_B65_K65"]
        w.use(b["field"])

        def state():
            return (ctx.occ_fetch().tobytes(), ctx.occ_distance_fetch(metres=False)[0].tobytes(), [a.tobytes() for a in ctx.occ_plan_fetch()],
                    ctx.occ_frontier_fetch().tobytes(), ctx.occ_distance_info().stale, ctx.occ_plan_info().stale, ctx.occ_frontier_info().stale,
                    [list(v) for v in (ctx.volume_shift_info().grid, ctx.volume_shift_info().field, ctx.volume_shift_info().plan)],
                    [a.tobytes() for a in ctx.occ_mcl_weigh(b["poses"], b["beams"], b["table"], capi.default_mcl_params(**b["mp"])).values()])

        before = state()
        pair = Pair(capi, ctx, cases.field(b["field"]))
        pair.set(b["poses"], 9)
        pair.move(np.array([0.1, 0.3, 0.0], F), np.array([0.02, 0.02, 0.02], F))
        pair.weigh(b["beams"], b["table"], **b["mp"])
        pair.resample(wtable_of(64), mode=2)
        assert state() == before
        # a field rebuild (another field), a recentre and lv_occ_configure leave the particles alone; a weigh reads the field as it stands
        held = pair.check()
        other = "planar" if b["field"] == "vol" else "vol"
        w.use(other)
        pair.ref.field = cases.field(other)
        pair.check()
        pair.weigh(b["beams"], b["table"], **b["mp"])
        ctx.occ_configure(capi.default_occupancy_params(**cases.PRM))
        got = ctx.lib.lv_occ_mcl_filter_weigh(ctx.h, C.byref(capi.default_mcl_params()), b["beams"].ctypes.data_as(C.POINTER(C.c_float)), len(b["beams"]),
                                              b["table"].ctypes.data_as(C.POINTER(C.c_uint32)), len(b["table"]), None)
        assert got == LV_ESTATE and "no distance field" in ctx.lib.lv_last_error().decode()
        kept = pair.check()                                      # (_get needs the grid alone)
        assert np.array_equal(kept["poses"].view(np.uint32), held["poses"].view(np.uint32))
        pair.move(np.array([0.0, 0.2, 0.0], F), np.array([0.0, 0.0, 0.0], F))   # (_move too)
        ctx.occ_load(cases.grid())
        w.name = None
        w.use(other)
        pair.weigh(b["beams"], b["table"], **b["mp"])
        pair.resample(wtable_of(64), mode=1)
        ctx.occ_mcl_filter_clear()
        assert ctx.occ_mcl_filter_info().set == 0
        ctx.occ_mcl_filter_clear()                               # (twice is fine)


def test_states_and_limits(capi):
    fptr, uptr = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
    poses, beams, table, wt = np.zeros((2, 4), F), np.zeros((3, 3), F), np.arange(4, dtype=np.uint32), np.array([3, 1], np.uint32)
    poses[:, :3] = [4.0, 1.0, 0.2]
    d, s = np.array([0.1, 0.2, 0.1], F), np.zeros(3, F)
    best, out3 = np.full(2, 7, np.int64), np.full((3, 4), 7, F)
    with capi.Context() as c:
        lib, h = c.lib, c.h
        stats = capi.MclFilterStats()
        mp, rp = capi.default_mcl_params(), capi.default_mcl_resample_params()
        calls = dict(set=lambda K=2: lib.lv_occ_mcl_filter_set(h, poses.ctypes.data_as(fptr), K, 1),
                     move=lambda: lib.lv_occ_mcl_filter_move(h, d.ctypes.data_as(fptr), s.ctypes.data_as(fptr)),
                     weigh=lambda B=3: lib.lv_occ_mcl_filter_weigh(h, C.byref(mp), beams.ctypes.data_as(fptr), B, table.ctypes.data_as(uptr), 4,
                                                                    best.ctypes.data_as(C.POINTER(C.c_int64))),
                     resample=lambda: lib.lv_occ_mcl_filter_resample(h, C.byref(rp), wt.ctypes.data_as(uptr), 2, C.byref(stats), None),
                     get=lambda cap=3: lib.lv_occ_mcl_filter_get(h, out3.ctypes.data_as(fptr), None, None, cap))

        def refused(name, what, code=LV_ESTATE, **kw):
            rc = calls[name](**kw)
            why = lib.lv_last_error().decode()
            assert rc == code and what in why, (name, rc, why)

        info = c.occ_mcl_filter_info()                           # zeros before _set; never LV_ESTATE
        assert (info.set, info.K, info.seed, info.epoch, info.since_resample) == (0, 0, 0, 0, 0)
        c.occ_mcl_filter_clear()
        for name in calls:
            refused(name, "lv_occ_configure")                    # before lv_occ_configure
        c.occ_configure(capi.default_occupancy_params(**cases.PRM))
        c.occ_load(cases.grid())
        refused("weigh", "no distance field")                    # the field before the particles
        refused("resample", "no distance field")
        refused("move", "no particles: call lv_occ_mcl_filter_set first")
        refused("get", "no particles: call lv_occ_mcl_filter_set first")
        assert calls["set"]() == LV_OK                           # _set needs the grid alone
        refused("weigh", "no distance field")
        c.occ_distance_build(capi.default_distance_params(**cases.DPS["planar"]))
        c.occ_mcl_filter_clear()
        refused("weigh", "no particles")
        refused("resample", "no particles")
        assert np.all(best == 7) and np.all(out3 == 7)
        assert c.occ_mcl_filter_info().set == 0
        for name in ("set", "move", "weigh", "resample", "get"):
            assert calls[name]() == LV_OK, (name, lib.lv_last_error().decode())
        info = c.occ_mcl_filter_info()
        assert (info.set, info.K, info.seed, info.epoch, info.since_resample) == (1, 2, 1, 2, 1 - stats.resampled)
        # the limits that need the particles: capacity below K, and K * B one past 2^30
        before = c.occ_mcl_filter_get()
        refused("get", "room for K", LV_EINVAL, cap=1)
        big = np.zeros((2 ** 20, 4), F)
        c.occ_mcl_filter_set(big, 0)
        refused("weigh", "K * B", LV_EINVAL, B=1025)
        info = c.occ_mcl_filter_info()
        assert (info.K, info.epoch, info.since_resample) == (2 ** 20, 0, 0)   # a refused call changes nothing
        # K = 2^20 itself runs: the largest block sums, the last index of every buffer
        big[:, :3] = [4.0, 1.0, 0.2]
        big[:, 3] = np.linspace(-3.0, 3.0, len(big), dtype=F)
        pair = Pair(capi, c, cases.field("planar"))
        pair.set(big, 2)
        pair.move(d, np.array([0.01, 0.01, 0.01], F))
        e1 = cases.random_batch(3, 1, 1)["beams"]
        pair.weigh(e1, table, out_cost=3, min_inside=0)          # (min_inside 0: every usable heading is eligible)
        st, anc = pair.resample(np.array([1 << 20, 1 << 19, 1], np.uint32), mode=2)
        assert st.resampled == 1 and st.n_eligible == 2 ** 20 and st.W >= 2 ** 20


# ---- the closed loop
def test_closed_loop_tracking(capi, world, lv):
    """mcl.DeviceFilter.track over the ten cycles of mcl_cases, K = 2048, from a Gaussian round the start: every cycle equals the
    reference filter bit for bit, and the last estimate lies within the measured bound of the truth."""
    from limo_velo_amd import mcl, occupancy

    truth = cases.true_poses()
    scans = [occupancy.simulate_scan(world.ctx, cases.yaw(p[3]), p[:3], cases.pattern()) for p in truth[1:]]
    assert all(np.array_equal(s, cases.ref_ranges(p)) for s, p in zip(scans, truth[1:]))
    table, wtable = cases.tables()
    p0 = mcl.gaussian_particles(cases.TRUE_START, 0.3, 0.15, cases.TRACK_K, np.random.default_rng(0))
    beams = [cases.scan_beams(r) for r in scans]
    got = mcl.DeviceFilter(world.use("planar"), p0, 0).track(cases.ODOMETRY, beams, table, wtable, alphas=cases.ALPHAS)
    want = mcl.DeviceFilter(fr.RefFilterContext(cases.field("planar")), p0, 0).track(cases.ODOMETRY, beams, table, wtable, alphas=cases.ALPHAS)
    assert len(got) == len(want) == 10 and len(got[0]["acc"]) == cases.TRACK_K == 2048
    for k, (g, w) in enumerate(zip(got, want)):
        for key in ("moved", "poses"):
            assert np.array_equal(g[key].view(np.uint32), w[key].view(np.uint32)), (k, key)
        assert np.array_equal(g["acc"], w["acc"]) and np.array_equal(g["n_in"], w["n_in"]) and np.array_equal(g["best"], w["best"]), k
        assert fr.stats_dict(g["stats"]) == fr.stats_dict(w["stats"]), k
        assert g["resampled"] == w["resampled"] and g["n_eff"] == w["n_eff"] and np.array_equal(g["estimate"], w["estimate"]), k
    assert sum(g["resampled"] for g in got) >= 3
    err_m, err_rad = cases.track_error(got)
    print("tracking error", err_m, "m", err_rad, "rad", "resamplings", sum(g["resampled"] for g in got))
    assert err_m <= TRACK_BOUND_M and err_rad <= TRACK_BOUND_RAD, (err_m, err_rad)
