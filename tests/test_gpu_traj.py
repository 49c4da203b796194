"""lv_traj_* (include/limovelo_hip.h "Trajectory") on the GPU, through capi, against tests/traj_ref.py on the scenes of
tests/traj_cases.py.

Bounds, all derived: f64 outputs (sample, smooth, correct, fetch) at 1e-9 * max(1, |ref|), the project's figure for f64 algebra across
two libms; an f32 output of register at half an f32 ulp of the reference's f64 value plus that term (one rounding plus the libm
difference); quaternions up to sign; "bit for bit" is array_equal on the raw bytes."""
import math

import numpy as np
import pytest

import cloud_messages as cm
import graph_cases as gcases
import graph_ref as gr
import traj_cases as cases
import traj_ref as tr

pytestmark = pytest.mark.gpu

IDENTITY = np.array([0, 0, 0, 0, 0, 0, 1.0])


@pytest.fixture(scope="module")
def capi(lv):
    from limo_velo_amd import capi as c

    return c


@pytest.fixture(scope="module")
def ctx(capi):
    with capi.Context() as c:
        yield c


def _bytes(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bytes(a), _bytes(b))


def _set(ctx, capi, times, poses):
    ctx.traj_set(capi.traj_knots(times, poses))


def _poses(k):
    return np.concatenate([k["t"], k["q"]], axis=1)


def _register(ctx, capi, xyz, at, layout=(32, 16), **prm):
    stride, toff = layout
    return ctx.traj_register((cases.records(xyz, at, stride, toff), stride, toff, len(xyz)), capi.default_traj_register_params(**prm))


def test_states(ctx, capi):
    LvError = capi.LvError
    ctx.traj_clear() if ctx.traj_info()["set"] else None
    assert ctx.traj_info()["set"] == 0
    calls = (lambda: ctx.traj_fetch(), lambda: ctx.traj_clear(), lambda: ctx.traj_sample([0.0]), lambda: ctx.traj_smooth(),
             lambda: ctx.traj_correct(capi.traj_knots([0.0], [IDENTITY])), lambda: _register(ctx, capi, cases.points(2), np.zeros(2)),
             lambda: _register(ctx, capi, cases.points(0), np.zeros(0)), lambda: ctx.traj_register_cloud(0.0, 1.0))

    def all_estate():
        for f in calls:
            with pytest.raises(LvError, match="error -4.*no trajectory"):
                f()

    all_estate()
    times, poses = cases.wander(9, seed=1)
    _set(ctx, capi, times, poses)
    info = ctx.traj_info()
    assert info["set"] == 1 and info["n"] == 9 and info["t_first"] == times[0] and info["t_last"] == times[-1]
    assert info["smooth_iterations"] == 0 and info["corrections"] == 0 and info["last_register"] == [0, 0, 0, 0]
    held = ctx.traj_fetch()
    assert _same(_poses(held), poses) and np.array_equal(held["time"], times)
    bad = poses.copy()
    bad[4, 2] = math.nan
    with pytest.raises(LvError, match="error -1.*knot 4"):
        _set(ctx, capi, times, bad)
    later = times.copy()
    later[3] = later[2]
    with pytest.raises(LvError, match="error -1.*knot 3.*time"):
        _set(ctx, capi, later, poses)
    assert _same(ctx.traj_fetch(), held)                 # a rejected set leaves the trajectory bit for bit
    with pytest.raises(LvError, match="error -1.*frame_time"):
        _register(ctx, capi, cases.points(2), times[:2], frame=capi.TRAJ_FRAME_AT, frame_time=times[-1] + 1.0)
    with pytest.raises(LvError, match="error -1.*frame_time"):
        _register(ctx, capi, cases.points(2), times[:2], frame=capi.TRAJ_FRAME_AT, frame_time=times[0] - 1e-9)
    ctx.traj_smooth(iterations=2)
    ctx.traj_correct(capi.traj_knots([0.0], [IDENTITY]))
    _, _, stats = _register(ctx, capi, cases.points(5), times[:5])
    info = ctx.traj_info()
    assert info["smooth_iterations"] == 2 and info["corrections"] == 1 and info["last_register"] == stats == [5, 0, 1, 0]
    _set(ctx, capi, times[:3], poses[:3])                # replaces; the counts start again
    info = ctx.traj_info()
    assert info["n"] == 3 and info["smooth_iterations"] == 0 and info["corrections"] == 0
    ctx.traj_clear()
    all_estate()


@pytest.mark.parametrize("n", cases.KNOT_COUNTS)
def test_sample_against_the_reference(ctx, capi, n):
    times, poses = cases.wander(n, seed=n)
    _set(ctx, capi, times, poses)
    at = np.concatenate([cases.point_times(times, 257, outside=2), times, [math.nan, math.inf, -math.inf]])
    for ex in (capi.TRAJ_CLAMP, capi.TRAJ_REFUSE):
        got, st = ctx.traj_sample(at, ex)
        want, wst = tr.sample(times, poses, at, ex)
        assert np.array_equal(st, wst)
        ok = ~np.isnan(want[:, 0])
        assert np.array_equal(np.isnan(got), np.isnan(want)) and tr.close_pose(got[ok], want[ok])
        own = slice(257, 257 + n)
        assert _same(got[own], poses) and np.all(st[own] == tr.INSIDE)       # a knot's own time: its pose bit for bit, the last too


def test_smooth_against_the_reference(ctx, capi):
    times, poses = cases.wander(300, seed=5)
    poses = cases.noisy(poses)
    fixed = np.zeros(300, bool)
    fixed[[7, 150, 298]] = True
    for kw, fx in ((dict(sigma=0.03, half_window=4, iterations=3, pin_ends=1), fixed), (dict(sigma=0.05, half_window=64, iterations=1, pin_ends=0), None),
                   (dict(sigma=0.03, half_window=4, iterations=0, pin_ends=1), fixed)):
        _set(ctx, capi, times, poses)
        ctx.traj_smooth(fixed=fx, **kw)
        got = ctx.traj_fetch()
        assert np.array_equal(got["time"], times)
        if kw["iterations"] == 0:
            assert _same(_poses(got), poses)
            continue
        want = tr.smooth(times, poses, kw["sigma"], kw["half_window"], kw["iterations"], bool(kw["pin_ends"]), fx)
        assert tr.close_pose(_poses(got), want) and tr.pose_distance(_poses(got), poses) > 1e-4
        held = ([0, 299] if kw["pin_ends"] else []) + ([] if fx is None else list(np.flatnonzero(fx)))
        assert _same(_poses(got)[held], poses[held])
        # the interval records follow the smoothed knots: sampling between knots agrees with the reference on them
        mid = 0.5 * (times[:-1] + times[1:])
        assert tr.close_pose(ctx.traj_sample(mid)[0], tr.sample(times, want, mid)[0])


def test_correct_against_the_reference(ctx, capi):
    times, poses = cases.wander(300, seed=6)
    rng = np.random.default_rng(8)
    ctimes = np.array([times[3], times[170] + 2.0 ** -9, times[280]])
    D = np.array([np.concatenate([rng.normal(0, 0.5, 3), gr.qexp(rng.normal(0, 0.3, 3))]) for _ in ctimes])
    _set(ctx, capi, times, poses)
    ctx.traj_correct(capi.traj_knots(ctimes, D))
    got = ctx.traj_fetch()
    want = tr.correct(times, poses, ctimes, D)
    assert np.array_equal(got["time"], times) and tr.close_pose(_poses(got), want)
    mid = 0.5 * (times[:-1] + times[1:])
    assert tr.close_pose(ctx.traj_sample(mid)[0], tr.sample(times, want, mid)[0])
    _set(ctx, capi, times, poses)
    ctx.traj_correct(capi.traj_knots(ctimes, np.tile(IDENTITY, (3, 1))))
    assert _same(_poses(ctx.traj_fetch()), poses)        # an identity correction leaves every bit
    with pytest.raises(capi.LvError, match="error -1.*correction: knot 1"):
        ctx.traj_correct(capi.traj_knots(ctimes[[0, 0]], D[:2]))


@pytest.mark.parametrize("n", cases.KNOT_COUNTS)
def test_register_shapes(ctx, capi, n):
    """every knot count against every point count, the layouts taking turns; both extrapolation modes"""
    times, poses = cases.wander(n, seed=20 + n)
    _set(ctx, capi, times, poses)
    for k, m in enumerate(cases.POINT_COUNTS):
        at = cases.point_times(times, m, seed=m, outside=2 if m >= 255 else 0)
        xyz = cases.points(m, seed=m)
        if m >= 255:
            at[100], xyz[101, 2], at[102] = math.nan, -math.inf, math.inf
        for ex in (capi.TRAJ_CLAMP, capi.TRAJ_REFUSE):
            layout = cases.LAYOUTS[(k + ex) % len(cases.LAYOUTS)]
            out, st, stats = _register(ctx, capi, xyz, at, layout, extrapolate=ex, ext_t=cases.EXTRINSIC[:3], ext_q=cases.EXTRINSIC[3:])
            want, wst = tr.register(times, poses, xyz, at, ex, cases.EXTRINSIC)
            assert np.array_equal(st, wst) and tr.close32(out, want), (n, m, ex, layout)
            assert stats[0] == (wst == tr.INSIDE).sum() and stats[1] == m - stats[0] and stats[2] + stats[3] == -(-m // tr.WG)
            assert (stats[2], stats[3]) == tr.routes(times, at)
    # count only
    out, st, stats2 = ctx.traj_register((cases.records(xyz, at, 32, 16), 32, 16, len(xyz)), capi.default_traj_register_params(extrapolate=ex),
                                        want_points=False, want_status=False)
    assert out is None and st is None and stats2[:2] == stats[:2]


def test_points_at_knot_times(ctx, capi):
    times, poses = cases.wander(tr.TILE + 1, seed=3)
    _set(ctx, capi, times, poses)
    xyz = cases.points(len(times))
    out, st, _ = _register(ctx, capi, xyz, times)
    assert np.all(st == tr.INSIDE)
    want = np.array([gr.rot(x[3:]) @ p.astype(float) + x[:3] for x, p in zip(poses, xyz)])   # the knot's own pose, the last included
    assert tr.close32(out, want)
    at = np.array([times[0] - 0.5, times[-1] + 0.5, math.nan, math.inf, -math.inf, times[0], times[-1]])
    for ex in (capi.TRAJ_CLAMP, capi.TRAJ_REFUSE):
        out, st, stats = _register(ctx, capi, xyz[:7], at, extrapolate=ex)
        assert list(st) == [tr.BEFORE, tr.AFTER, tr.NONFINITE, tr.NONFINITE, tr.NONFINITE, tr.INSIDE, tr.INSIDE] and stats[:2] == [2, 5]
        assert np.all(np.isnan(out[2:5])) and not np.isnan(out[5:]).any()
        if ex == capi.TRAJ_CLAMP:
            ends = np.array([gr.rot(x[3:]) @ p.astype(float) + x[:3] for x, p in zip(poses[[0, -1]], xyz[:2])])
            assert tr.close32(out[:2], ends)
        else:
            assert np.all(np.isnan(out[:2]))


def test_routes_give_the_same_bits(ctx, capi):
    n, m = 2 * tr.TILE + 3, 1000
    times, poses = cases.wander(n, seed=2)
    _set(ctx, capi, times, poses)
    at = cases.point_times(times, m, outside=3)
    xyz = cases.points(m)
    at[400], xyz[401, 0] = math.nan, math.nan
    prm = dict(ext_t=cases.EXTRINSIC[:3], ext_q=cases.EXTRINSIC[3:], extrapolate=capi.TRAJ_REFUSE)
    out, st, stats = _register(ctx, capi, xyz, at, **prm)
    assert stats[2:] == [4, 0]                                    # sorted: tile-route workgroups only
    want, wst = tr.register(times, poses, xyz, at, tr.REFUSE, cases.EXTRINSIC)
    assert np.array_equal(st, wst) and tr.close32(out, want)
    out2, st2, stats2 = _register(ctx, capi, xyz, at, **prm)
    assert _same(out2, out) and _same(st2, st) and stats2 == stats   # a second call repeats the first call's bits
    perm = np.random.default_rng(3).permutation(m)
    outp, stp, statsp = _register(ctx, capi, xyz[perm], at[perm], **prm)
    assert statsp[2:] == [0, 4] and statsp[:2] == stats[:2]       # shuffled: search-route workgroups
    back = np.empty(m, int)
    back[perm] = np.arange(m)
    assert _same(outp[back], out) and _same(stp[back], st)
    ctx.set_option("traj_tile", 0)
    try:
        out0, st0, stats0 = _register(ctx, capi, xyz, at, **prm)
    finally:
        ctx.set_option("traj_tile", 1)
    assert stats0[2:] == [0, 4] and _same(out0, out) and _same(st0, st)
    assert _register(ctx, capi, xyz, at, **prm)[2] == stats


def test_times_stay_f64(ctx, capi):
    n, m = 2 * tr.TILE + 3, 1000
    times, poses = cases.wander(n, seed=4)
    at = cases.point_times(times, m, outside=2)
    xyz = cases.points(m)
    assert np.array_equal(times * 1024, np.round(times * 1024)) and np.array_equal(at * 1024, np.round(at * 1024))
    res = []
    for shift in (0.0, 2.0 ** 30):
        assert np.array_equal((times + shift) - shift, times) and np.array_equal((at + shift) - shift, at)
        _set(ctx, capi, times + shift, poses)
        for tile in (1, 0):
            ctx.set_option("traj_tile", tile)
            try:
                res.append(_register(ctx, capi, xyz, at + shift, layout=(24, 12), ext_t=cases.EXTRINSIC[:3], ext_q=cases.EXTRINSIC[3:]))
            finally:
                ctx.set_option("traj_tile", 1)
        res.append(_register(ctx, capi, xyz, at + shift, frame=capi.TRAJ_FRAME_AT, frame_time=float(at[500] + shift)))
    assert float(np.float32(2.0 ** 30 + at[500])) != 2.0 ** 30 + at[500]      # f32 does not hold these stamps
    for a, b in zip(res[:3], res[3:]):
        assert _same(a[0], b[0]) and _same(a[1], b[1]) and a[2] == b[2]
    assert (res[0][1] == tr.INSIDE).sum() == m - 4


def test_half_turns_and_frame_at(ctx, capi):
    times, poses = cases.half_turns()
    _set(ctx, capi, times, poses)
    at = np.linspace(times[0], times[-1], 257)
    xyz = cases.points(257)
    out, st, _ = _register(ctx, capi, xyz, at)
    want, _ = tr.register(times, poses, xyz, at)
    assert np.all(st == tr.INSIDE) and tr.close32(out, want)
    got, _ = ctx.traj_sample(at)
    assert tr.close_pose(got, tr.sample(times, poses, at)[0])
    flipped = poses.copy()
    flipped[:, 3:] *= np.array([1, -1, 1, 1, -1.0])[:, None]
    _set(ctx, capi, times, flipped)
    assert tr.close32(_register(ctx, capi, xyz, at)[0], want)      # a knot stored as -q: the same rotation
    times, poses = cases.wander(40, seed=12)
    _set(ctx, capi, times, poses)
    at = cases.point_times(times, 300)
    xyz = cases.points(300)
    for ft in (float(times[17]), float(0.25 * times[17] + 0.75 * times[18]), float(times[0]), float(times[-1])):
        prm = dict(ext_t=cases.EXTRINSIC[:3], ext_q=cases.EXTRINSIC[3:], frame=capi.TRAJ_FRAME_AT, frame_time=ft)
        out, st, _ = _register(ctx, capi, xyz, at, **prm)
        want, wst = tr.register(times, poses, xyz, at, tr.CLAMP, cases.EXTRINSIC, tr.FRAME_AT, ft)
        assert np.array_equal(st, wst) and tr.close32(out, want), ft
    for ft in (float(times[0]) - 2.0 ** -10, float(times[-1]) + 2.0 ** -10, math.nan, math.inf):
        with pytest.raises(capi.LvError, match="error -1.*frame_time"):
            _register(ctx, capi, xyz, at, frame=capi.TRAJ_FRAME_AT, frame_time=ft)


def test_graph_consistency(ctx, capi):
    """After correct with a solved graph's corrections, points stamped at keyframe times land where lv_graph_warp_points puts the
    same points.  The warp takes world points W (f32); register is handed the same W with the extrinsic E = T_0^-1 of the
    keyframe, so both compute D_k W in f64 from the same exact inputs and round once: one f32 ulp plus 1e-9 between them."""
    from limo_velo_amd import offline

    g, _ = gcases.ring12()                           # a drifted start: the solve moves every free node
    start = g["poses"].copy()
    ctx.graph_set(start, g["fixed"], g["edges"], g["priors"])
    ctx.graph_optimise(**gcases.SOLVE)
    now = ctx.graph_fetch()
    assert gr.distance(now, start) > 1e-3 and np.array_equal(now[0], start[0])
    n = len(start)
    kt = 10.0 + 0.5 * np.arange(n)

    class Solved:
        states = [np.concatenate([p, np.zeros(19)]) for p in start]
        poses = now

    D = offline.corrections(Solved, kt)
    assert np.array_equal(D["q"][0], [0, 0, 0, 1]) and np.array_equal(D["t"][0], [0, 0, 0])   # the fixed node: the identity, exactly
    _set(ctx, capi, kt, start)                       # the knots: the keyframes as they stood before the solve
    ctx.traj_correct(D)
    got = ctx.traj_fetch()
    assert tr.close_pose(_poses(got), now) and _same(_poses(got)[0], start[0])
    worst = 0.0
    for k in range(n):
        W = cases.points(20, seed=90 + k)
        warped = ctx.graph_warp_points(W, np.full(20, k, np.uint32))
        R0 = gr.rot(start[k, 3:])
        out, st, _ = _register(ctx, capi, W, np.full(20, kt[k]), ext_t=-(R0.T @ start[k, :3]), ext_q=gr.qconj(start[k, 3:]))
        assert np.all(st == tr.INSIDE)
        bound = np.spacing(np.abs(warped)).astype(float) + tr.TOL * np.maximum(1.0, np.abs(warped))
        worst = max(worst, float((np.abs(out.astype(float) - warped.astype(float)) / bound).max()))
    print("graph consistency: worst |register - warp| / (one f32 ulp + 1e-9)", worst)
    assert worst <= 1.0
    ctx.graph_clear()


def test_register_cloud_equals_register_on_the_fetched_window(ctx, capi):
    raw, fmt, stamp = cm.make_message("hesai", 1500, seed=4)
    f = capi.CloudFormat(fmt["point_step"], fmt["off_x"], fmt["off_y"], fmt["off_z"], fmt["off_time"], fmt["time_type"], fmt["off_intensity"],
                         fmt["intensity_type"], fmt["off_range"], fmt["range_type"], fmt["relative_time"])
    ctx.cloud_clear(math.inf)
    kept = ctx.cloud_ingest(raw, 1500, f, capi.IngestParams(stamp, 0, 0, 0.1, 1, 0.5))
    size = ctx.cloud_size()
    assert kept == size == 1500
    allpts = ctx.cloud_fetch(-math.inf, math.inf)
    t0, t1 = float(allpts["time"][0]), float(allpts["time"][-1])
    knot_t = t0 + (t1 - t0) * np.linspace(0.1, 0.9, 2 * tr.TILE + 3)      # the window's ends lie outside the trajectory
    _, poses = cases.wander(len(knot_t), seed=8)
    _set(ctx, capi, knot_t, poses)
    prm = capi.default_traj_register_params(extrapolate=capi.TRAJ_REFUSE, ext_t=cases.EXTRINSIC[:3], ext_q=cases.EXTRINSIC[3:])
    for a, b in ((-math.inf, math.inf), (t0 + 0.3 * (t1 - t0), t0 + 0.6 * (t1 - t0)), (t1 + 1.0, t1 + 2.0)):
        window = ctx.cloud_fetch(a, b)
        want = ctx.traj_register(window, prm)
        got = ctx.traj_register_cloud(a, b, prm)
        assert len(got[0]) == len(window) and _same(got[0], want[0]) and _same(got[1], want[1]) and got[2] == want[2]
    assert len(allpts) == 1500 and (want[2] == [0, 0, 0, 0])
    full = ctx.traj_register_cloud(-math.inf, math.inf, prm)
    assert full[2][0] > 1000 and full[2][1] > 100 and np.isnan(full[0][full[1] != tr.INSIDE]).all()
    assert ctx.cloud_size() == size and _same(ctx.cloud_fetch(-math.inf, math.inf), allpts)   # nothing in the buffer changed
    ctx.cloud_clear(math.inf)


def test_offline_pass(ctx, capi):
    """offline.remap on a seeded room scanned from a moving sensor; knots at a tenth of the point rate carry a step at every second one"""
    from limo_velo_amd import offline

    sc = cases.room_scan()
    at, xyz, kt, stepped = sc["point_times"], sc["xyz"], sc["knot_times"], sc["stepped"]
    E = cases.EXTRINSIC
    sweeps = []
    for s in sc["sweeps"]:
        rec = np.zeros(s.stop - s.start, capi.POINT_DTYPE)
        rec["x"], rec["y"], rec["z"], rec["time"] = xyz[s, 0], xyz[s, 1], xyz[s, 2], at[s]
        sweeps.append(rec)
    smooth = dict(sigma=2.0 ** -6, half_window=4, iterations=2, pin_ends=1)

    # the reference pass on the same inputs: rigid per keyframe (every sweep at the knot nearest its middle), interpolated, smoothed
    def rigid(poses):
        out = []
        for s in sc["sweeps"]:
            T = poses[np.argmin(np.abs(kt - at[(s.start + s.stop) // 2]))]
            M = gr.rot(T[3:]) @ gr.rot(E[3:])
            out.append(xyz[s].astype(float) @ M.T + gr.rot(T[3:]) @ E[:3] + T[:3])
        return np.concatenate(out)

    ref_rigid = cases.room_distance(rigid(stepped))
    ref_interp_pts, _ = tr.register(kt, stepped, xyz, at, tr.REFUSE, E)
    ref_interp = cases.room_distance(ref_interp_pts)
    smoothed = tr.smooth(kt, stepped, smooth["sigma"], smooth["half_window"], smooth["iterations"], True)
    ref_smooth_pts, _ = tr.register(kt, smoothed, xyz, at, tr.REFUSE, E)
    ref_smooth = cases.room_distance(ref_smooth_pts)
    print("offline pass, RMS distance to the room's surfaces (reference): rigid", ref_rigid, "interpolated", ref_interp, "smoothed", ref_smooth)
    assert ref_interp <= ref_rigid and ref_smooth <= ref_interp

    # the device: rigid placement through FRAME-less registration against a one-knot trajectory per sweep
    dev_rigid = []
    for s, rec in zip(sc["sweeps"], sweeps):
        k = int(np.argmin(np.abs(kt - at[(s.start + s.stop) // 2])))
        _set(ctx, capi, kt[k:k + 1], stepped[k:k + 1])
        dev_rigid.append(ctx.traj_register(rec, capi.default_traj_register_params(ext_t=E[:3], ext_q=E[3:]))[0])
    d_rigid = cases.room_distance(np.concatenate(dev_rigid))
    _set(ctx, capi, kt, stepped)
    world = offline.remap(ctx, sweeps, E, chunk=1024)
    assert tr.close32(world, ref_interp_pts) and ctx.map_size() > 0
    d_interp = cases.room_distance(world)
    ctx.traj_smooth(**smooth)
    world_s = offline.remap(ctx, sweeps, E, chunk=1024)
    assert tr.close32(world_s, ref_smooth_pts)
    d_smooth = cases.room_distance(world_s)
    print("offline pass, RMS distance to the room's surfaces (device): rigid", d_rigid, "interpolated", d_interp, "smoothed", d_smooth)
    assert abs(d_rigid - ref_rigid) <= 1e-6 and abs(d_interp - ref_interp) <= 1e-6 and abs(d_smooth - ref_smooth) <= 1e-6
    assert d_interp <= d_rigid and d_smooth <= d_interp
