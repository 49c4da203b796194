"""Seeded scenes shared by the trajectory tests (TEST INFRASTRUCTURE): trajectories, point records in the layouts lv_traj_register
takes, and the room scanned from a moving sensor of the offline pass."""
import math

import numpy as np

import graph_ref as gr
import traj_ref as tr

KNOT_COUNTS = (1, 2, 3, tr.TILE, tr.TILE + 1, 2 * tr.TILE + 3)
POINT_COUNTS = (0, 1, 255, 256, 257, 1000)
LAYOUTS = ((20, 12), (24, 16), (32, 16), (24, 12))   # (stride, time_offset); offset 12 is unaligned for an f64


def wander(n, seed=0, dt=1.0 / 64, t0=0.0):
    """n knots on a smooth, wandering path; times are multiples of 2^-10 s (dt must be one): (times, poses)"""
    rng = np.random.default_rng(seed)
    times = t0 + dt * np.arange(n) + (rng.integers(0, 4, n) * 2.0 ** -10 if n > 1 else 0.0)
    ph = rng.uniform(0, 2 * math.pi, 6)
    poses = np.zeros((n, 7))
    for k, t in enumerate(times - t0):
        poses[k, :3] = [3.0 * math.sin(0.7 * t + ph[0]) + 1.5 * t, 2.0 * math.cos(0.5 * t + ph[1]), 0.5 * math.sin(0.9 * t + ph[2])]
        poses[k, 3:] = gr.qexp(np.array([0.3 * math.sin(0.8 * t + ph[3]), 0.2 * math.cos(0.6 * t + ph[4]), 0.9 * t + ph[5]]))
    return times, poses


def point_times(times, m, seed=1, outside=0):
    """m point times, multiples of 2^-10 s, ascending, spread over the trajectory; `outside` of them before and as many after"""
    rng = np.random.default_rng(seed)
    lo, hi = times[0], times[-1]
    span = max(hi - lo, 2.0 ** -6)
    t = np.sort(np.round((lo + rng.uniform(0, 1, m) * span) * 1024.0) / 1024.0)
    t = np.clip(t, lo, max(hi, lo))
    if outside and m >= 2 * outside:
        t[:outside] = lo - 2.0 ** -4 * (1 + np.arange(outside))[::-1]
        t[m - outside:] = max(hi, lo) + 2.0 ** -4 * (1 + np.arange(outside))
    return t


def points(m, seed=2):
    return np.random.default_rng(seed).uniform(-20, 20, (m, 3)).astype(np.float32)


def records(xyz, at, stride, time_offset):
    """the bytes of m records: x, y, z f32 at 0, the f64 time at time_offset, the rest 0xA5"""
    m = len(xyz)
    raw = np.full((m, stride), 0xA5, np.uint8)
    raw[:, :12] = np.ascontiguousarray(xyz, np.float32).view(np.uint8).reshape(m, 12)
    raw[:, time_offset:time_offset + 8] = np.ascontiguousarray(at, np.float64).view(np.uint8).reshape(m, 8)
    return raw.reshape(-1).tobytes()


def noisy(poses, seed=3, sigma_t=0.02, sigma_r=0.01):
    rng = np.random.default_rng(seed)
    out = np.array(poses, float)
    for k in range(len(out)):
        out[k, :3] += rng.normal(0, sigma_t, 3)
        out[k, 3:] = tr.normalise(gr.qmul(out[k, 3:], gr.qexp(rng.normal(0, sigma_r, 3))))
    return out


def half_turns():
    """five knots whose neighbours stand 179 degrees apart about z; knots 2 and 3 are stored with the opposite sign"""
    times = np.arange(5) * 0.5
    poses = np.zeros((5, 7))
    for k in range(5):
        poses[k, :3] = [k, 0.5 * k, 0.0]
        poses[k, 3:] = gr.qexp(np.array([0.0, 0.0, math.radians(179.0) * k]))
    poses[2, 3:] *= -1.0
    poses[3, 3:] *= -1.0
    return times, poses


# ---- the offline pass: a room scanned from a moving sensor
ROOM = np.array([[-6.0, 6.0], [-4.0, 4.0], [0.0, 3.0]])   # the six planes x = -6, 6; y = -4, 4; z = 0, 3
EXTRINSIC = np.concatenate([[0.1, -0.05, 0.2], gr.qexp(np.array([0.02, -0.03, 0.5]))])


def room_truth(times):
    """the body's true pose at times: a slow drive through the room, turning"""
    out = np.zeros((len(times), 7))
    for k, t in enumerate(times):
        out[k, :3] = [-2.0 + 1.0 * t, 0.5 * math.sin(0.8 * t), 1.0 + 0.1 * math.sin(1.3 * t)]
        out[k, 3:] = gr.qexp(np.array([0.05 * math.sin(t), 0.04 * math.cos(1.1 * t), 0.6 * t]))
    return out


def room_scan(n_points=3000, n_sweeps=3, seed=5):
    """Raw returns in the sensor frame, generated from the true trajectory: dict with
    point_times [n], xyz [n, 3] f32 (sensor frame), sweeps: list of slices, knot_times, truth (poses at the knots), stepped
    (the knots with a step added at every second one)."""
    rng = np.random.default_rng(seed)
    at = np.arange(n_points) * 2.0 ** -10               # ~1 kHz points over ~3 s
    truth_pts = room_truth(at)
    ER, Et = gr.rot(EXTRINSIC[3:]), EXTRINSIC[:3]
    xyz = np.zeros((n_points, 3), np.float32)
    for k in range(n_points):
        R, p = gr.rot(truth_pts[k, 3:]), truth_pts[k, :3]
        Rl, o = R @ ER, R @ Et + p                      # the sensor in the world
        d = rng.normal(size=3)
        d /= np.linalg.norm(d)
        dw = Rl @ d
        best = math.inf
        for ax in range(3):                             # the nearest wall along the ray
            for wall in ROOM[ax]:
                if abs(dw[ax]) > 1e-9:
                    s = (wall - o[ax]) / dw[ax]
                    if 1e-6 < s < best:
                        best = s
        xyz[k] = (d * best).astype(np.float32)
    knot_times = at[::10].copy()                        # a tenth of the point rate
    knot_times = np.append(knot_times, at[-1] + 2.0 ** -10 * 10)
    truth = room_truth(knot_times)
    stepped = truth.copy()
    stepped[1::2, :3] += np.array([0.03, -0.02, 0.01])
    for k in range(1, len(stepped), 2):
        stepped[k, 3:] = tr.normalise(gr.qmul(stepped[k, 3:], gr.qexp(np.array([0.0, 0.0, 0.01]))))
    edges = np.linspace(0, n_points, n_sweeps + 1).astype(int)
    sweeps = [slice(int(a), int(b)) for a, b in zip(edges[:-1], edges[1:])]
    return dict(point_times=at, xyz=xyz, sweeps=sweeps, knot_times=knot_times, truth=truth, stepped=stepped)


def room_distance(world):
    """RMS distance of world points to the nearest of the room's six planes"""
    w = np.asarray(world, float).reshape(-1, 3)
    d = np.min(np.stack([np.abs(w[:, ax] - wall) for ax in range(3) for wall in ROOM[ax]]), axis=0)
    return float(math.sqrt(np.mean(d * d)))
