"""The rule of include/limovelo_hip.h "Surface registration" restated in numpy (TEST INFRASTRUCTURE): f64 throughout, every
operation in the header's order, so that sample() gives the device's bits (only + - * / and floor occur).  The sums of an
evaluation run over the source points one after the other; the device adds them as a tree, which is what the 1e-9 bounds of the
device tests cover.  A volume is dict(origin [3], resolution, nx, ny, nz, S, W) with S, W int32 [nz, ny, nx].
tests/test_surf_align_ref.py checks the reference against itself; the host build of lv_surf_align.hpp and the device are held to it."""
import math

import numpy as np

import graph_ref as gr
import ndt_ref as nr

F = np.float32
EPS = 2.0 ** -52
OUTSIDE, UNKNOWN, KNOWN = 0, 1, 2
CONVERGED, MAX_ITERATIONS, NO_OVERLAP = 0, 1, 2
CHUNK = 512
U_LIMIT = 2.0 ** 24
ALIGN = dict(min_weight=1, max_iterations=50, min_points=6, max_dist=0.4, huber=0.1, step_tol=1e-6, lambda_init=1e-4, lambda_min=1e-10,
             lambda_max=1e8)
TRIU = np.triu_indices(6)


def sample(vol, x, min_weight=1):
    """(d [n] metres, n [n, 3], status [n] uint8) at world points x [n, 3] f64; zeros where the status is not KNOWN"""
    x = np.asarray(x, np.float64).reshape(-1, 3)
    o = np.asarray(vol["origin"], F).astype(np.float64)
    r = float(F(vol["resolution"]))
    dims = (vol["nx"], vol["ny"], vol["nz"])
    S, W = np.asarray(vol["S"]).reshape(-1), np.asarray(vol["W"]).reshape(-1)
    m = len(x)
    with np.errstate(all="ignore"):
        u = (x - o) / r - 0.5
        ok = np.all(np.abs(u) < U_LIMIT, axis=1)      # (a NaN compares false)
        u = np.where(ok[:, None], u, 0.0)
        fl = np.floor(u)
    i = fl.astype(np.int64)
    f = u - fl
    for a in range(3):
        ok &= (i[:, a] >= 0) & (i[:, a] + 1 <= dims[a] - 1)
    status = np.where(ok, KNOWN, OUTSIDE).astype(np.uint8)
    i = np.where(ok[:, None], i, 0)
    at = (i[:, 2] * dims[1] + i[:, 1]) * dims[0] + i[:, 0]
    phi = np.zeros((m, 2, 2, 2))                       # [a, b, c]
    known = ok.copy()
    for c in range(2):
        for b in range(2):
            for a in range(2):
                k = at + a + b * dims[0] + c * dims[0] * dims[1]
                w = W[k]
                known &= w >= min_weight
                phi[:, a, b, c] = S[k].astype(np.float64) / np.where(w >= 1, w, 1).astype(np.float64)
    status[ok & ~known] = UNKNOWN
    fx, fy, fz = f[:, 0, None, None], f[:, 1, None], f[:, 2]
    e2 = phi[:, 1] - phi[:, 0]                          # [b, c]
    c2 = phi[:, 0] + fx * e2
    ey = c2[:, 1] - c2[:, 0]                            # [c]
    c1 = c2[:, 0] + fy * ey
    ex = e2[:, 0] + fy * (e2[:, 1] - e2[:, 0])
    gz = c1[:, 1] - c1[:, 0]
    val = c1[:, 0] + fz * gz
    gx = ex[:, 0] + fz * (ex[:, 1] - ex[:, 0])
    gy = ey[:, 0] + fz * (ey[:, 1] - ey[:, 0])
    d = np.where(known, (r / 256.0) * val, 0.0)
    n = np.where(known[:, None], np.stack([gx / 256.0, gy / 256.0, gz / 256.0], axis=1), 0.0)
    return d, n, status


def rho(d, h):
    """(rho, w) of residuals d under the Huber width h (0: quadratic)"""
    d = np.asarray(d, np.float64)
    a = np.abs(d)
    quad = (a <= h) | (h == 0.0)
    with np.errstate(all="ignore"):
        w = np.where(quad, 1.0, h / np.where(quad, 1.0, a))
    return np.where(quad, 0.5 * d * d, h * (a - 0.5 * h)), w


def gate_rho(max_dist, huber):
    return float(rho(np.array([max_dist]), huber)[0][0])


def transform(src, pose):
    """x = R p + t in f64, the rows summed as the header sums them; also p (f64) and R"""
    p = np.asarray(src, F).reshape(-1, 3).astype(np.float64)
    R, t = gr.rot(pose[3:]), np.asarray(pose[:3], float)
    x = np.stack([((R[k, 0] * p[:, 0] + R[k, 1] * p[:, 1]) + R[k, 2] * p[:, 2]) + t[k] for k in range(3)], axis=1)
    return x, p, R


def terms(vol, src, pose, min_weight=1, max_dist=0.4, huber=0.1):
    """(rows [n, 28]: what each source point adds, IN [n] bool)"""
    x, p, R = transform(src, pose)
    n_pts = len(p)
    d, n, status = sample(vol, x, min_weight)
    with np.errstate(all="ignore"):
        inn = (status == KNOWN) & (np.abs(d) <= max_dist)
    r, w = rho(d, huber)
    zero = np.zeros(n_pts)
    P = [[zero, -p[:, 2], p[:, 1]], [p[:, 2], zero, -p[:, 0]], [-p[:, 1], p[:, 0], zero]]
    A = [[-((R[i, 0] * P[0][j] + R[i, 1] * P[1][j]) + R[i, 2] * P[2][j]) for j in range(3)] for i in range(3)]
    J = [n[:, 0], n[:, 1], n[:, 2]] + [(n[:, 0] * A[0][c] + n[:, 1] * A[1][c]) + n[:, 2] * A[2][c] for c in range(3)]
    wJ = [w * J[a] for a in range(6)]
    wd = w * d
    rows = np.stack([wJ[a] * J[b] for a, b in zip(*TRIU)] + [wd * J[a] for a in range(6)] + [r], axis=1)
    return rows, inn


def evaluate(vol, src, pose, min_weight=1, max_dist=0.4, huber=0.1, reverse=False):
    """(acc [28]: the 21 of H, the 6 of g, E; n_in) at pose [7]"""
    if len(np.asarray(src).reshape(-1, 3)) == 0:
        return np.zeros(28), 0
    rows, inn = terms(vol, src, pose, min_weight, max_dist, huber)
    rows = rows[inn]
    if reverse:
        rows = rows[::-1]
    acc = np.cumsum(rows, axis=0)[-1] if len(rows) else np.zeros(28)      # (one row after the other)
    return acc, int(inn.sum())


def cost_of(E, n_src, n_in, max_dist, huber):
    return float(E + float(n_src - n_in) * gate_rho(max_dist, huber))


def accept(c_new, c_old):
    return c_new <= c_old + 64.0 * EPS * abs(c_old)


def align_one(vol, src, guess, reverse=False, **kw):
    """The loop of the header from one guess: dict(pose, cost, info, n_in, status, accepted, rejected, last_step, lambda) and
    costs: the cost at the guess and after every accepted step"""
    a = dict(ALIGN, **kw)
    ev = lambda pose: evaluate(vol, src, pose, a["min_weight"], a["max_dist"], a["huber"], reverse)
    n_src = len(np.asarray(src).reshape(-1, 3))
    x = np.array(guess, float)
    acc, n_in = ev(x)
    out = dict(pose=x, cost=0.0, info=np.zeros(21), n_in=0, status=NO_OVERLAP, accepted=0, rejected=0, last_step=0.0, costs=[])
    out["lambda"] = a["lambda_init"]
    if n_in < a["min_points"]:
        return out
    lam, cur, status, last = a["lambda_init"], acc, MAX_ITERATIONS, 0.0
    cost = cost_of(cur[27], n_src, n_in, a["max_dist"], a["huber"])
    costs = [cost]
    accepted = rejected = 0
    for _ in range(a["max_iterations"]):
        d = nr.solve(cur[:21], cur[21:27], lam)
        step = float(np.max(np.abs(d))) if np.all(np.isfinite(d)) else math.inf
        xt = gr.retract(x, d) if math.isfinite(step) else x
        new, n_new = ev(xt)
        c_new = cost_of(new[27], n_src, n_new, a["max_dist"], a["huber"])
        if math.isfinite(step) and n_new >= a["min_points"] and accept(c_new, cost):
            x, cur, n_in, cost = xt, new, n_new, c_new
            costs.append(cost)
            accepted += 1
            last = step
            lam = max(lam / 3.0, a["lambda_min"])
            if step <= a["step_tol"]:
                status = CONVERGED
                break
        else:
            rejected += 1
            lam = min(4.0 * lam, a["lambda_max"])
    out.update(pose=x, cost=cost, info=cur[:21].copy(), n_in=n_in, status=status, accepted=accepted, rejected=rejected, last_step=last, costs=costs)
    out["lambda"] = lam
    return out


def best_of(results):
    b = (-1, -1)
    for k, r in enumerate(results):
        if r["status"] != NO_OVERLAP and (b[0] < 0 or r["cost"] < results[b[0]]["cost"]):
            b = (k, r["n_in"])
    return b


def align(vol, src, guesses, reverse=False, **kw):
    res = [align_one(vol, src, g, reverse, **kw) for g in guesses]
    return res, best_of(res)


pose_distance = nr.pose_distance
