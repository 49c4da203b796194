"""The trajectory rule of include/limovelo_hip.h "Trajectory" restated in numpy f64 on graph_ref's algebra (TEST INFRASTRUCTURE):
sample, smooth, correct, register, the bracket search and the knot range of a chunk.  tests/test_traj_ref.py holds it to closed
forms; the host build of lv_traj.hpp and the device are held to it.

A trajectory is (times [n], poses [n, 7]) with a pose (t, q = x y z w)."""
import math

import numpy as np

import graph_ref as gr

INSIDE, BEFORE, AFTER, NONFINITE = 0, 1, 2, 3
CLAMP, REFUSE = 0, 1
WORLD, FRAME_AT = 0, 1
TILE = 256
WG = 256
KNOT_DTYPE = np.dtype([("time", "f8"), ("t", "f8", 3), ("q", "f8", 4)])
assert KNOT_DTYPE.itemsize == 64
TOL = 1e-9   # f64 algebra across two libms (tests/test_graph_host.py)


def knots(times, poses):
    x = np.asarray(poses, float).reshape(-1, 7)
    k = np.zeros(len(x), KNOT_DTYPE)
    k["time"], k["t"], k["q"] = times, x[:, :3], x[:, 3:]
    return k


def unpack(k):
    return np.array(k["time"], float), np.concatenate([k["t"], k["q"]], axis=1)


def normalise(q):
    return q / math.sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3])


def bracket(times, t):
    """the first index whose time is > t"""
    return int(np.searchsorted(times, t, side="right"))


def sample_one(times, poses, t, extrapolate=CLAMP):
    """(pose [7], status)"""
    nan = np.full(7, np.nan)
    if not math.isfinite(t):
        return nan, NONFINITE
    n = len(times)
    ub = bracket(times, t)
    if ub == 0:
        return (poses[0].copy() if extrapolate == CLAMP else nan), BEFORE
    i = ub - 1
    if t == times[i]:
        return poses[i].copy(), INSIDE
    if i == n - 1:
        return (poses[i].copy() if extrapolate == CLAMP else nan), AFTER
    a, b = poses[i], poses[i + 1]
    u = (t - times[i]) / (times[i + 1] - times[i])
    w = gr.qlog(gr.qmul(gr.qconj(a[3:]), b[3:]))
    q = normalise(gr.qmul(a[3:], gr.qexp(u * w)))
    return np.concatenate([a[:3] + u * (b[:3] - a[:3]), q]), INSIDE


def sample(times, poses, at, extrapolate=CLAMP):
    out = [sample_one(times, poses, float(t), extrapolate) for t in np.asarray(at, float).reshape(-1)]
    return np.array([o[0] for o in out]).reshape(-1, 7), np.array([o[1] for o in out], np.uint8)


def smooth(times, poses, sigma, half_window, iterations, pin_ends=True, fixed=None):
    x = np.array(poses, float)
    n = len(x)
    for _ in range(iterations):
        nxt = x.copy()
        for i in range(n):
            if (fixed is not None and fixed[i]) or (pin_ends and i in (0, n - 1)):
                continue
            W, sp, sw = 0.0, np.zeros(3), np.zeros(3)
            for j in range(max(0, i - half_window), min(n - 1, i + half_window) + 1):
                d = (times[j] - times[i]) / sigma
                w = math.exp(-0.5 * (d * d))
                W += w
                sp += w * (x[j, :3] - x[i, :3])
                sw += w * gr.qlog(gr.qmul(gr.qconj(x[i, 3:]), x[j, 3:]))
            nxt[i, :3] = x[i, :3] + sp / W
            nxt[i, 3:] = normalise(gr.qmul(x[i, 3:], gr.qexp(sw / W)))
        x = nxt
    return x


def is_identity(D):
    return bool(np.all(D[:3] == 0.0) and np.all(D[3:6] == 0.0) and D[6] == 1.0)


def correct(times, poses, ctimes, cposes):
    out = np.array(poses, float)
    for i in range(len(out)):
        D, _ = sample_one(ctimes, cposes, float(times[i]), CLAMP)
        if is_identity(D):
            continue
        out[i, :3] = gr.rot(D[3:]) @ out[i, :3] + D[:3]
        out[i, 3:] = normalise(gr.qmul(D[3:], out[i, 3:]))
    return out


def frame_map(times, poses, frame_time, ext):
    """(F_R, F_t) of (T(frame_time) E)^-1"""
    T, _ = sample_one(times, poses, frame_time, CLAMP)
    M = gr.rot(T[3:]) @ gr.rot(ext[3:])
    m = gr.rot(T[3:]) @ ext[:3] + T[:3]
    return M.T, -(M.T @ m)


def register(times, poses, xyz, at, extrapolate=CLAMP, ext=None, frame=WORLD, frame_time=0.0):
    """(out [n, 3] f64 BEFORE the rounding to f32, status [n]); xyz [n, 3] f32, at [n] f64"""
    ext = np.array([0, 0, 0, 0, 0, 0, 1.0]) if ext is None else np.asarray(ext, float)
    ER = gr.rot(ext[3:])
    F = frame_map(times, poses, frame_time, ext) if frame == FRAME_AT else None
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    out, st = np.full((len(xyz), 3), np.nan), np.zeros(len(xyz), np.uint8)
    for k in range(len(xyz)):
        T, s = sample_one(times, poses, float(at[k]), extrapolate)
        p = xyz[k].astype(float)
        if not np.all(np.isfinite(p)) or s == NONFINITE:
            st[k] = NONFINITE
            continue
        st[k] = s
        if np.isnan(T[0]):
            continue
        w = gr.rot(T[3:]) @ (ER @ p + ext[:3]) + T[:3]
        out[k] = w if F is None else F[0] @ w + F[1]
    return out, st


def tile_range(times, t_min, t_max):
    """[k_lo, k_end) of a chunk whose finite times span [t_min, t_max]; (0, 0) when it has none (t_min > t_max)"""
    if not t_min <= t_max:
        return 0, 0
    ub_min, ub_max = bracket(times, t_min), bracket(times, t_max)
    return max(ub_min - 1, 0), min(ub_max + 1, len(times))


def routes(times, at, tile=True):
    """(tile workgroups, search workgroups) of a register call over the point times `at`"""
    at = np.asarray(at, float)
    nt = ns = 0
    for off in range(0, len(at), WG):
        c = at[off:off + WG]
        f = c[np.isfinite(c)]
        lo, end = tile_range(times, f.min(), f.max()) if len(f) else (0, 0)
        if tile and end - lo <= TILE:
            nt += 1
        else:
            ns += 1
    return nt, ns


# ---- the bounds
def close64(got, want):
    got, want = np.asarray(got, float), np.asarray(want, float)
    return got.shape == want.shape and bool(np.all((np.abs(got - want) <= TOL * np.maximum(1.0, np.abs(want))) | (np.isnan(got) & np.isnan(want))))


def close_pose(got, want):
    """poses [.., 7]: positions at TOL, quaternions up to sign"""
    got, want = np.asarray(got, float).reshape(-1, 7), np.asarray(want, float).reshape(-1, 7)
    if got.shape != want.shape:
        return False
    sg = np.where(np.sum(got[:, 3:] * want[:, 3:], axis=1) < 0, -1.0, 1.0)[:, None]
    return close64(got[:, :3], want[:, :3]) and close64(sg * got[:, 3:], want[:, 3:])


def f32_bound(want, ulps=0.5):
    """half an f32 ulp of the f64 reference (one rounding) plus the libm term"""
    want = np.asarray(want, float)
    return ulps * np.spacing(np.abs(want).astype(np.float32)).astype(float) + TOL * np.maximum(1.0, np.abs(want))


def close32(got, want, ulps=0.5):
    got, want = np.asarray(got, np.float32), np.asarray(want, float)
    if got.shape != want.shape:
        return False
    nan = np.isnan(want)
    if not np.array_equal(np.isnan(got), nan):
        return False
    return bool(np.all(np.abs(got.astype(float) - want)[~nan] <= f32_bound(want[~nan], ulps)))


# ---- closed forms
def screw(times, p0, v, q0, axis, rate):
    """constant velocity and a constant rotation rate about a fixed body axis: poses [n, 7]"""
    axis = np.asarray(axis, float) / np.linalg.norm(axis)
    out = np.zeros((len(times), 7))
    for k, t in enumerate(times):
        out[k, :3] = np.asarray(p0, float) + np.asarray(v, float) * t
        out[k, 3:] = normalise(gr.qmul(np.asarray(q0, float), gr.qexp(rate * t * axis)))
    return out


def pose_distance(a, b):
    """max over poses of |dt| and of |Log(Ra^T Rb)|"""
    a, b = np.asarray(a, float).reshape(-1, 7), np.asarray(b, float).reshape(-1, 7)
    dt = np.linalg.norm(a[:, :3] - b[:, :3], axis=1)
    dr = np.array([np.linalg.norm(gr.qlog(gr.qmul(gr.qconj(x[3:]), y[3:]))) for x, y in zip(a, b)])
    return float(max(dt.max(), dr.max()))
