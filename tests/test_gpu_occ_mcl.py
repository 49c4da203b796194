"""lv_occ_mcl_weigh (include/limovelo_hip.h "Localisation") on the GPU, through capi, against tests/mcl_ref.py: equality on every
score, on every n_in and on `best`, no tolerance.  The world, the fields and the batches are those of tests/mcl_cases.py (a room of
40 x 30 x 3 cells loaded with lv_occ_load; B = 1, 3, 63, 64, 65, 130 and 300, so every group width and its tail; K = 0, 1, 2, 63, 64,
65, 257; tables of 1, 2 and 4096 entries; a truncated and a signed field; end points on and just past the field's faces; unusable
headings; min_inside; a sum past 2^32; ties); then a field after lv_volume_recentre, what the call must leave alone, the states it
refuses, and the closed loop of limo_velo_amd.mcl.

The tracking bound of test_closed_loop_tracking is measured, not guessed (DESIGN.md "Localisation"): the reference filter alone,
seeds 0..4, ends 0.0744, 0.0755, 0.0667, 0.0772, 0.0727 m and 0.0307, 0.0285, 0.0269, 0.0271, 0.0298 rad from the truth; twice the
worst is 0.154 m and 0.061 rad, below the floor of one cell (0.25 m) and one step of the ranking test's heading table (10 degrees),
so the floor is the bound."""
import ctypes as C

import numpy as np
import pytest

import mcl_cases as cases
import mcl_ref as mr

pytestmark = pytest.mark.gpu

LV_OK, LV_EINVAL, LV_ESTATE = 0, -1, -4
F = np.float32
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


def _run(capi, ctx, b, want=("score", "n_in", "best")):
    return ctx.occ_mcl_weigh(b["poses"], b["beams"], b["table"], capi.default_mcl_params(**b["mp"]), want)


def _same(got, want, name=""):
    for k in got:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (name, k, np.nonzero(got[k] != want[k])[0][:8])


@pytest.mark.parametrize("name", sorted(cases.batches(), key=lambda n: (cases.batches()[n]["field"], n)))
def test_case_against_the_reference(capi, world, name):
    b = cases.batches()[name]
    got = _run(capi, world.use(b["field"]), b)
    assert set(got) == {"score", "n_in", "best"}
    _same(got, cases.answers()[name], name)


def test_the_cases_do_what_they_are_for():
    cases.check_the_cases_do_what_they_are_for()


def test_outputs_asked_for_one_at_a_time_and_the_same_call_twice(capi, world):
    for name in ("random_B130_K257", "random_B3_K65", "overflow", "ties", "none_eligible", "headings"):
        b, want = cases.batches()[name], cases.answers()[name]
        ctx = world.use(b["field"])
        first = _run(capi, ctx, b)
        for keys in (("score",), ("n_in",), ("best",), ("score", "best"), ("n_in", "best")):
            got = _run(capi, ctx, b, keys)
            assert set(got) == set(keys)
            _same(got, want, name)
        again = _run(capi, ctx, b)
        for k in first:
            assert first[k].tobytes() == again[k].tobytes(), (name, k)


def test_a_field_after_a_recentre(capi):
    import recentre_ref as rcr

    d = (3, -2, 0)
    with capi.Context() as c:
        w = World(capi, c)
        for name in ("planar", "vol"):
            b = cases.random_batch(11, 130, 65, fname=name, out_cost=3)
            before = _run(capi, w.use(name), b)
            _same(before, mr.weigh(cases.field(name), b["mp"], b["poses"], b["beams"], b["table"]), name)
            c.volume_recentre(capi.LV_VOLUME_OCC, d)
            assert c.occ_distance_info().stale == 1 and not any(c.volume_shift_info().field)
            _same(_run(capi, c, b), before, name + ": the stale field lies where it was built")
            c.occ_distance_build(capi.default_distance_params(**cases.DPS[name]))
            assert list(c.volume_shift_info().field) == list(d)
            f = cases.field(name, d)
            assert np.array_equal(c.occ_distance_fetch(metres=False)[0], f["s2"])
            assert np.array_equal(np.array([v for v in c.occ_params().origin], F), rcr.origin_at(cases.PRM["origin"], d, cases.RES))
            after = _run(capi, c, b)
            _same(after, mr.weigh(f, b["mp"], b["poses"], b["beams"], b["table"]), name + ": rebuilt")
            assert np.any(after["score"] != before["score"])
            c.volume_recentre(capi.LV_VOLUME_OCC, tuple(-v for v in d))
            c.occ_load(cases.grid())
            w.name = None


def test_nothing_else_changes(capi, world):
    ctx = world.use("planar")
    ctx.occ_plan_build(np.array([[6.0, -1.0, 0.0]], F), np.array([250, 120, 40, 10, 3, 1], np.uint8), capi.default_plan_params(connectivity=8, min_clear_s2=2))
    ctx.occ_frontier_build(capi.default_frontier_params(planar=1, k_lo=0, k_hi=2, connectivity=8))

    def state():
        return (ctx.occ_fetch().tobytes(), ctx.occ_distance_fetch(metres=False)[0].tobytes(), [a.tobytes() for a in ctx.occ_plan_fetch()],
                ctx.occ_frontier_fetch().tobytes(), ctx.occ_distance_info().stale, ctx.occ_plan_info().stale, ctx.occ_frontier_info().stale,
                [list(v) for v in (ctx.volume_shift_info().grid, ctx.volume_shift_info().field, ctx.volume_shift_info().plan)])

    before = state()
    for name in ("random_B130_K257", "random_B1_K1", "edges_planar", "overflow"):
        b = cases.batches()[name]
        if b["field"] == "planar":
            _run(capi, ctx, b)
    assert state() == before


def _raw(capi, ctx, K=2, B=3, n_table=4, **mp):
    """A raw call with arrays of at most a few elements whatever K, B and n_table say: only for calls that must be refused, or
    whose K, B and n_table are the small defaults."""
    fptr, uptr = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
    small = K <= 2 and B <= 3 and n_table <= 4
    p = capi.default_mcl_params(**mp)
    poses, beams, table = np.zeros((2, 4), F), np.zeros((3, 3), F), np.arange(4, dtype=np.uint32)
    score, n_in, best = np.full(2, 7, np.uint64), np.full(2, 7, np.uint32), np.full(2, 7, np.int64)
    rc = ctx.lib.lv_occ_mcl_weigh(ctx.h, C.byref(p), poses.ctypes.data_as(fptr), K, beams.ctypes.data_as(fptr), B, table.ctypes.data_as(uptr), n_table,
                                  score.ctypes.data_as(C.POINTER(C.c_uint64)), n_in.ctypes.data_as(uptr), best.ctypes.data_as(C.POINTER(C.c_int64)))
    assert small or rc != LV_OK
    untouched = bool(np.all(score == 7) and np.all(n_in == 7) and np.all(best == 7))
    return rc, untouched, ctx.lib.lv_last_error().decode()


def test_states_and_limits(capi):
    with capi.Context() as c:
        rc, untouched, why = _raw(capi, c)
        assert (rc, untouched) == (LV_ESTATE, True) and "lv_occ_configure" in why          # before lv_occ_configure
        c.occ_configure(capi.default_occupancy_params(**cases.PRM))
        c.occ_load(cases.grid())
        rc, untouched, why = _raw(capi, c)
        assert (rc, untouched) == (LV_ESTATE, True) and "no distance field" in why          # before a build
        assert _raw(capi, c, K=0)[:2] == (LV_ESTATE, True)                                  # (K = 0 too: the states come first)
        c.occ_distance_build(capi.default_distance_params(**cases.DPS["planar"]))
        assert _raw(capi, c)[:2] == (LV_OK, False)
        # every limit one past its end, with a context that would answer
        for kw, what in ((dict(K=2 ** 20 + 1), "K: 0..2^20"), (dict(B=0), "B: 1..65536"), (dict(B=65537), "B: 1..65536"), (dict(K=2 ** 20, B=1025), "K * B"),
                         (dict(n_table=0), "n_table"), (dict(n_table=4097), "n_table"), (dict(out_cost=2 ** 24 + 1), "out_cost"),
                         (dict(min_inside=-1), "min_inside"), (dict(min_inside=4), "min_inside")):
            rc, untouched, why = _raw(capi, c, **kw)
            assert (rc, untouched) == (LV_EINVAL, True) and what in why, (kw, why)
        # K = 0 writes best only
        out = c.occ_mcl_weigh(np.zeros((0, 4), F), np.zeros((3, 3), F), np.arange(4, dtype=np.uint32))
        assert list(out["best"]) == [-1, -1] and len(out["score"]) == 0 and len(out["n_in"]) == 0
        # a stale field is used as it is
        c.occ_load(np.full_like(cases.grid(), -1.0))
        assert c.occ_distance_info().stale == 1
        b = cases.batches()["random_B65_K65"]
        f = b["field"]
        c.occ_load(cases.grid())
        c.occ_distance_build(capi.default_distance_params(**cases.DPS[f]))
        c.occ_load(np.full_like(cases.grid(), -1.0))
        assert c.occ_distance_info().stale == 1
        _same(_run(capi, c, b), cases.answers()["random_B65_K65"], "stale")
        assert c.occ_distance_info().stale == 1
        c.occ_distance_clear()
        assert _raw(capi, c)[:2] == (LV_ESTATE, True)
        # lv_occ_configure frees the buffers and the field
        c.occ_distance_build(capi.default_distance_params())
        assert _raw(capi, c)[0] == LV_OK
        c.occ_configure(capi.default_occupancy_params(**cases.PRM))
        assert _raw(capi, c)[:2] == (LV_ESTATE, True)


# ---- the closed loop
def _device_scans(world, poses):
    from limo_velo_amd import occupancy

    return [occupancy.simulate_scan(world.ctx, cases.yaw(p[3]), p[:3], cases.pattern()) for p in poses]


def test_closed_loop_ranking(capi, world, lv):
    """The true pose scores no worse than any pose more than 2 cells or 10 degrees away, on the planar and the 3-D field; the
    scene and the table are checked on the references alone first."""
    from limo_velo_amd import mcl

    table, _ = cases.tables()
    poses, true, far = cases.ranking_poses()
    assert far.sum() > 400 and not far[true]
    ranges = cases.ref_ranges(cases.TRUE_START)
    assert np.isfinite(ranges).sum() >= 100
    beams = cases.scan_beams(ranges)
    for name in ("planar", "vol"):
        want = mcl.weigh(mr.RefContext(cases.field(name)), poses, beams, table)
        assert want["score"][true] != np.uint64(mr.NO_SCORE) and np.all(want["score"][true] <= want["score"][far]), name   # the references alone
        (scan,) = _device_scans(world, [cases.TRUE_START])
        assert np.array_equal(scan, ranges)
        got = mcl.weigh(world.use(name), poses, cases.scan_beams(scan), table)
        _same(got, want, name)
        assert np.all(got["score"][true] <= got["score"][far])


def test_closed_loop_tracking(capi, world, lv):
    """track() over ten cycles, K = 2048, from a Gaussian round the start: every cycle's device scores are the reference's, bit for
    bit, and the last estimate lies within the measured bound of the truth."""
    truth = cases.true_poses()
    scans = _device_scans(world, truth[1:])
    assert all(np.array_equal(s, cases.ref_ranges(p)) for s, p in zip(scans, truth[1:]))
    got = cases.run_track(world.use("planar"), scans, 0)
    want = cases.run_track(mr.RefContext(cases.field("planar")), scans, 0)
    assert len(got) == len(want) == 10 and len(got[0]["score"]) == cases.TRACK_K == 2048
    for k, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g["moved"].view(np.uint32), w["moved"].view(np.uint32)), k
        assert np.array_equal(g["score"], w["score"]) and np.array_equal(g["n_in"], w["n_in"]) and np.array_equal(g["best"], w["best"]), k
        assert g["resampled"] == w["resampled"] and g["n_eff"] == w["n_eff"], k
    assert any(g["resampled"] for g in got)
    err_m, err_rad = cases.track_error(got)
    print("tracking error", err_m, "m", err_rad, "rad")
    assert err_m <= TRACK_BOUND_M and err_rad <= TRACK_BOUND_RAD, (err_m, err_rad)
