"""tests/traj_ref.py, the numpy restatement of the trajectory rule (include/limovelo_hip.h "Trajectory"), held to closed forms:
constant velocity with a constant rotation rate samples onto the analytic pose, that trajectory is a fixed point of the smoother
away from the ends, smoothing a noisy copy brings it closer to the truth, and the corrections of two keyframes reproduce each
keyframe's rigid correction at its own time."""
import math

import numpy as np

import graph_ref as gr
import traj_cases as cases
import traj_ref as tr

P0, V, Q0, AXIS, RATE = [1.0, -2.0, 0.5], [0.8, 0.3, -0.1], gr.qexp(np.array([0.2, -0.1, 0.4])), [0.3, -0.5, 0.8], 0.7


def test_screw_motion_samples_onto_the_analytic_pose():
    times = np.arange(21) * 0.25
    poses = tr.screw(times, P0, V, Q0, AXIS, RATE)
    at = np.random.default_rng(0).uniform(times[0], times[-1], 200)
    got, st = tr.sample(times, poses, at)
    want = tr.screw(at, P0, V, Q0, AXIS, RATE)
    assert np.all(st == tr.INSIDE)
    sg = np.where(np.sum(got[:, 3:] * want[:, 3:], axis=1) < 0, -1.0, 1.0)[:, None]
    assert np.abs(got[:, :3] - want[:, :3]).max() <= 1e-12 and np.abs(sg * got[:, 3:] - want[:, 3:]).max() <= 1e-12


def test_knot_times_sides_and_signs():
    times, poses = cases.wander(7, seed=4)
    got, st = tr.sample(times, poses, times)
    assert np.array_equal(got, poses) and np.all(st == tr.INSIDE)            # bit for bit, the last knot included
    at = [times[0] - 1.0, times[-1] + 1.0, math.nan, math.inf, -math.inf]
    got, st = tr.sample(times, poses, at, tr.CLAMP)
    assert list(st) == [tr.BEFORE, tr.AFTER, tr.NONFINITE, tr.NONFINITE, tr.NONFINITE]
    assert np.array_equal(got[0], poses[0]) and np.array_equal(got[1], poses[-1]) and np.all(np.isnan(got[2:]))
    got, st = tr.sample(times, poses, at, tr.REFUSE)
    assert list(st) == [tr.BEFORE, tr.AFTER, tr.NONFINITE, tr.NONFINITE, tr.NONFINITE] and np.all(np.isnan(got))
    one, st = tr.sample(times[:1], poses[:1], [times[0] - 1, times[0], times[0] + 1])
    assert np.array_equal(one, np.repeat(poses[:1], 3, axis=0)) and list(st) == [tr.BEFORE, tr.INSIDE, tr.AFTER]
    # a knot stored as -q gives the same rotation, and 179 degrees between neighbours go the short way
    ht, hp = cases.half_turns()
    flipped = hp.copy()
    flipped[2:4, 3:] *= -1.0
    mid = 0.5 * (ht[:-1] + ht[1:])
    a, b = tr.sample(ht, hp, mid)[0], tr.sample(ht, flipped, mid)[0]
    assert tr.pose_distance(a, b) <= 1e-12
    for k, x in enumerate(a):   # half of 179 degrees from the knot before
        assert abs(np.linalg.norm(gr.qlog(gr.qmul(gr.qconj(hp[k, 3:]), x[3:]))) - math.radians(89.5)) <= 1e-12


def test_screw_motion_is_a_fixed_point_of_the_smoother_away_from_the_ends():
    times = np.arange(41) * 0.1
    poses = tr.screw(times, P0, V, Q0, AXIS, RATE)
    hw = 5
    out = tr.smooth(times, poses, sigma=0.25, half_window=hw, iterations=3, pin_ends=False)
    inner = slice(3 * hw, len(times) - 3 * hw)    # three iterations carry the ends' asymmetry 3 hw knots inwards
    assert tr.pose_distance(out[inner], poses[inner]) <= 1e-12
    assert tr.pose_distance(out[:hw], poses[:hw]) > 1e-6      # the ends' windows are one-sided: they do move
    pinned = tr.smooth(times, poses, sigma=0.25, half_window=hw, iterations=3, pin_ends=True)
    assert np.array_equal(pinned[0], poses[0]) and np.array_equal(pinned[-1], poses[-1])
    assert np.array_equal(tr.smooth(times, poses, 0.25, hw, 0), poses)


def test_smoothing_a_noisy_copy_brings_it_closer_to_the_truth():
    times = np.arange(81) * 0.05
    truth = tr.screw(times, P0, V, Q0, AXIS, RATE)
    noisy = cases.noisy(truth, seed=7)
    fixed = np.zeros(len(times), bool)
    fixed[40] = True
    out = tr.smooth(times, noisy, sigma=0.15, half_window=8, iterations=2, pin_ends=True, fixed=fixed)

    # Away from the ends (two iterations carry the one-sided windows' lag 2 half_window knots inwards; a kernel smoother is biased
    # there by about sigma times the speed, far above this noise).  Inside, the truth is a fixed point and white noise shrinks by
    # sqrt(sum w^2) / sum w = 0.31 per iteration at sigma = 3 knots: 0.6 leaves room for the one fixed knot and the sample's luck.
    inner = slice(16, len(times) - 16)

    def rms(x):
        dt = (x[:, :3] - truth[:, :3])[inner]
        dr = np.array([gr.qlog(gr.qmul(gr.qconj(a[3:]), b[3:])) for a, b in zip(truth, x)])[inner]
        return math.sqrt(np.mean(np.sum(dt * dt, axis=1))), math.sqrt(np.mean(np.sum(dr * dr, axis=1)))

    (t0, r0), (t1, r1) = rms(noisy), rms(out)
    print("rms before", t0, r0, "after", t1, r1)
    assert t1 < 0.6 * t0 and r1 < 0.6 * r0
    assert np.array_equal(out[40], noisy[40]) and np.array_equal(out[0], noisy[0]) and np.array_equal(out[-1], noisy[-1])


def test_corrections_of_two_keyframes_reproduce_each_rigid_correction():
    times, poses = cases.wander(30, seed=9)
    rng = np.random.default_rng(11)
    kf = [4, 22]
    ctimes = times[kf]
    D = np.array([np.concatenate([rng.normal(0, 0.5, 3), gr.qexp(rng.normal(0, 0.2, 3))]) for _ in kf])
    out = tr.correct(times, poses, ctimes, D)
    for k, d in zip(kf, D):   # at a keyframe's own time: exactly its rigid correction
        want_t = gr.rot(d[3:]) @ poses[k, :3] + d[:3]
        want_q = tr.normalise(gr.qmul(d[3:], poses[k, 3:]))
        assert np.abs(out[k, :3] - want_t).max() <= 1e-12 and np.abs(out[k, 3:] - want_q).max() <= 1e-12
    # clamped outside the keyframes: the first correction before, the second behind
    assert np.abs(out[0, :3] - (gr.rot(D[0, 3:]) @ poses[0, :3] + D[0, :3])).max() <= 1e-12
    assert np.abs(out[-1, :3] - (gr.rot(D[1, 3:]) @ poses[-1, :3] + D[1, :3])).max() <= 1e-12
    # between them the correction turns gradually: no step at any knot
    assert np.array_equal(tr.correct(times, poses, ctimes, np.tile([0, 0, 0, 0, 0, 0, 1.0], (2, 1))), poses)


def test_register_and_the_routes():
    times, poses = cases.wander(2 * tr.TILE + 3, seed=2)
    at = cases.point_times(times, 1000, outside=3)
    xyz = cases.points(1000)
    out, st = tr.register(times, poses, xyz, at)
    assert (st == tr.BEFORE).sum() == 3 and (st == tr.AFTER).sum() == 3 and not np.isnan(out).any()
    out, st = tr.register(times, poses, xyz, at, tr.REFUSE)
    assert np.isnan(out[st != tr.INSIDE]).all() and not np.isnan(out[st == tr.INSIDE]).any()
    # FRAME_AT: a point stamped at frame_time comes back as it was measured (E and T cancel)
    ft = float(at[500])
    same = np.flatnonzero(at == ft)
    out, _ = tr.register(times, poses, xyz, at, ext=cases.EXTRINSIC, frame=tr.FRAME_AT, frame_time=ft)
    assert np.abs(out[same] - xyz[same]).max() <= 1e-12
    assert tr.routes(times, at) == (4, 0)
    perm = np.random.default_rng(3).permutation(1000)
    assert tr.routes(times, at[perm]) == (0, 4) and tr.routes(times, at, tile=False) == (0, 4)
    assert tr.tile_range(times, math.inf, -math.inf) == (0, 0)
    assert tr.tile_range(times, times[0] - 2, times[0] - 1) == (0, 1) and tr.tile_range(times, times[-1] + 1, times[-1] + 2) == (len(times) - 1, len(times))
