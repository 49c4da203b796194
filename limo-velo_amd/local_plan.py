"""The local planner on top of lv_occ_rollout (include/limovelo_hip.h "Rollouts"): what base_local_planner / dwa_local_planner and
nav2's MPPI controller do with a global plan.  footprint_points() samples a rectangular robot's outline, dwa_controls() the
dynamic window, rollout() runs candidate control sequences on the device and returns the records as a dict of arrays, dwa() picks
the best constant command, mppi() does one sampling update of a nominal sequence, and drive() closes the loop: it asks a step
function for a command and advances the pose by the rule's own step until the goal is near.

Every function takes the context as its first argument and uses nothing of it but occ_rollout(), so the same code runs against
anything that answers like capi.Context.occ_rollout."""
from __future__ import annotations

import math

import numpy as np

from . import capi

NO_SCORE = np.uint64(2 ** 64 - 1)
DEFAULT_LIMITS = dict(v_min=0.0, v_max=0.5, w_min=-1.0, w_max=1.0, acc_v=0.5, acc_w=2.0)


def _params(params, kw) -> capi.RolloutParams:
    """A copy of params (None: the defaults) with the fields kw overrides."""
    p = capi.RolloutParams.from_buffer_copy(params if params is not None else capi.default_rollout_params())
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def footprint_points(length: float, width: float, spacing: float) -> np.ndarray:
    """[n, 2] f32 body-frame points on the outline of a length x width rectangle centred on the robot's origin, x forward: the
    four corners and, on every side, samples at most `spacing` apart.  At most 64 (ValueError beyond: widen the spacing)."""
    if not (length > 0 and width > 0 and spacing > 0):
        raise ValueError("footprint_points: length, width and spacing > 0")
    hx, hy = 0.5 * float(length), 0.5 * float(width)
    corners = [(hx, hy), (-hx, hy), (-hx, -hy), (hx, -hy)]
    pts = []
    for (ax, ay), (bx, by) in zip(corners, corners[1:] + corners[:1]):
        n = max(1, math.ceil(math.hypot(bx - ax, by - ay) / float(spacing)))
        pts += [(ax + (bx - ax) * t / n, ay + (by - ay) * t / n) for t in range(n)]
    if len(pts) > 64:
        raise ValueError(f"footprint_points: {len(pts)} points, lv_occ_rollout takes at most 64")
    return np.array(pts, np.float32)


def dwa_controls(v: float, w: float, limits=None, nv: int = 7, nw: int = 15, window: float = 0.5) -> np.ndarray:
    """[nv * nw, 1, 2] f32 constant commands (v, w) on a regular lattice over the dynamic window: what the robot can reach from
    the velocity (v, w) within `window` seconds under limits = dict(v_min, v_max, w_min, w_max, acc_v, acc_w), clipped to the
    velocity limits.  v runs slowest."""
    lim = dict(DEFAULT_LIMITS, **(limits or {}))
    v_lo, v_hi = max(lim["v_min"], v - lim["acc_v"] * window), min(lim["v_max"], v + lim["acc_v"] * window)
    w_lo, w_hi = max(lim["w_min"], w - lim["acc_w"] * window), min(lim["w_max"], w + lim["acc_w"] * window)
    vs = np.linspace(min(v_lo, v_hi), v_hi, int(nv))
    ws = np.linspace(min(w_lo, w_hi), w_hi, int(nw))
    return np.stack(np.meshgrid(vs, ws, indexing="ij"), axis=-1).reshape(-1, 1, 2).astype(np.float32)


def rollout(ctx, pose, controls, params: capi.RolloutParams | None = None, footprint=None, poses: bool = False, **kw) -> dict:
    """lv_occ_rollout of controls [K, Tc, 2] from pose (x, y, th); kw overrides fields of params (T, dt, weights, ...).  Returns
    a dict of the record's fields as [K] arrays, "score" [K] uint64 (2^64 - 1: not eligible), "best" (index or -1), "best_score",
    and with poses=True "poses" [K, T + 1, 3] (NaN rows past "steps")."""
    p = _params(params, kw)
    want = ("results", "score", "best") + (("poses",) if poses else ())
    got = ctx.occ_rollout(pose, controls, p, footprint, want)
    out = {f: got["results"][f] for f in got["results"].dtype.names}
    out.update(score=got["score"], best=int(got["best"][0]), best_score=int(got["best"][1]))
    if poses:
        out["poses"] = got["poses"]
    return out


def dwa(ctx, pose, vel=(0.0, 0.0), limits=None, nv: int = 7, nw: int = 15, window: float = 0.5, params=None, footprint=None, **kw) -> dict:
    """One cycle of the dynamic window approach: the commands of dwa_controls(*vel, ...) rolled out, the best by the device's
    `best`.  Returns dict(cmd: (v, w) f32 or None when no command is eligible, index, score, controls)."""
    u = dwa_controls(float(vel[0]), float(vel[1]), limits, nv, nw, window)
    p = _params(params, kw)
    best = ctx.occ_rollout(pose, u, p, footprint, ("best",))["best"]
    i = int(best[0])
    return dict(cmd=None if i < 0 else (u[i, 0, 0], u[i, 0, 1]), index=i, score=int(best[1]), controls=u)


def mppi(ctx, pose, nominal, sigma, K: int, lam: float, rng: np.random.Generator, params=None, footprint=None, **kw):
    """One MPPI update of the nominal sequence nominal [T, 2]: K sequences, the first the nominal itself and the others with
    Gaussian noise of standard deviation sigma (v, w) from rng, are scored on the device; the new nominal is their average under
    the soft-min weights exp(-(score - least) / lam), over the eligible ones, in f64 on the host.  Returns (new nominal [T, 2] f64,
    the best sequence's index); with no eligible sequence (the old nominal, -1)."""
    nominal = np.asarray(nominal, np.float64).reshape(-1, 2)
    T = len(nominal)
    noise = rng.normal(size=(int(K), T, 2)) * np.asarray(sigma, np.float64).reshape(1, 1, 2)
    noise[0] = 0.0
    u = (nominal[None] + noise).astype(np.float32)
    p = _params(params, kw)
    p.T = T
    got = ctx.occ_rollout(pose, u, p, footprint, ("score", "best"))
    ok = got["score"] != NO_SCORE
    if not ok.any():
        return nominal, -1
    s = got["score"][ok].astype(np.float64)
    wgt = np.exp(-(s - s.min()) / float(lam))
    wgt /= wgt.sum()
    return np.tensordot(wgt, u[ok].astype(np.float64), axes=1), int(got["best"][0])


def advance(ctx, pose, cmd, dt: float):
    """The pose one step of dt seconds on under cmd = (v, w), by the rule's own arithmetic (a rollout of one sequence and one
    step, without a footprint); None when that pose is bad (outside the plan or in a blocked cell)."""
    p = capi.default_rollout_params(T=1, dt=float(dt), min_steps=0)
    got = ctx.occ_rollout(pose, np.array(cmd, np.float32).reshape(1, 1, 2), p, None, ("results", "poses"))
    return got["poses"][0, 1].copy() if got["results"]["steps"][0] == 1 else None


def drive(ctx, pose, step_fn, n_iter: int, goal=None, goal_tol: float = 0.0, dt: float = 0.1) -> dict:
    """The closed loop: up to n_iter times, step_fn(ctx, pose, vel) -> (v, w) or None, then the pose advances by advance().  Stops
    when step_fn has no command, when the advance is refused, or when goal (x, y) is given and the pose is within goal_tol of it.
    Returns dict(poses [n + 1, 3] f32, the start included, cmds [n, 2] f32, reached: bool)."""
    pose = np.asarray(pose, np.float32).reshape(3).copy()
    poses, cmds, vel = [pose], [], (np.float32(0), np.float32(0))

    def near(q):
        return goal is not None and math.hypot(float(q[0]) - float(goal[0]), float(q[1]) - float(goal[1])) <= goal_tol

    reached = near(pose)
    for _ in range(int(n_iter)):
        if reached:
            break
        cmd = step_fn(ctx, pose, vel)
        if cmd is None:
            break
        nxt = advance(ctx, pose, cmd, dt)
        if nxt is None:
            break
        pose, vel = nxt, cmd
        poses.append(pose)
        cmds.append(cmd)
        reached = near(pose)
    return dict(poses=np.array(poses, np.float32), cmds=np.array(cmds, np.float32).reshape(-1, 2), reached=bool(reached))
