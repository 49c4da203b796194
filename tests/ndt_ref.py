"""The NDT rule of include/limovelo_hip.h "NDT registration" restated in numpy (TEST INFRASTRUCTURE): int64 moments, f64 otherwise.
reverse=True sums the source points of an evaluation in reversed order: what the loop's outcome owes to the order of a sum shows
as the difference between the two.  tests/test_ndt_ref.py checks the reference against itself; the host build of lv_ndt.hpp and
the device are held to it."""
import math

import numpy as np

import graph_ref as gr
import occupancy_ref as oref

F = np.float32
EPS = 2.0 ** -52
CONVERGED, MAX_ITERATIONS, NO_OVERLAP = 0, 1, 2
CHUNK = 512
D2_DEFAULT = 0.43312300470355464
PARAMS = dict(origin=(-64.0, -64.0, -8.0), resolution=1.0, nx=128, ny=128, nz=16, min_points=5, reg=0.01)
ALIGN = dict(search=7, max_iterations=100, d2=D2_DEFAULT, step_tol=1e-6, lambda_init=1e-4, lambda_min=1e-10, lambda_max=1e8)
S2_PAIRS = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
TRIU = np.triu_indices(6)
OFFSETS = np.array([(0, 0, 0), (1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)], np.int64)


def gauss_d2(resolution=1.0, outlier_ratio=0.55):
    """Magnusson's d2 (PCL's gauss_d2_)"""
    c1 = 10.0 * (1.0 - outlier_ratio)
    c2 = outlier_ratio / resolution ** 3
    d3 = -math.log(c2)
    d1 = -math.log(c1 + c2) - d3
    return -2.0 * math.log((-math.log(c1 * math.exp(-0.5) + c2) - d3) / d1)


def params(**kw):
    return dict(PARAMS, **kw)


def voxel_of(prm, pts):
    """(ok [n], c [n, 3] int64, r [n, 3] int64) of f32 points: the build's assignment"""
    qf = oref.quant_f(np.asarray(pts, F).reshape(-1, 3), prm["origin"], prm["resolution"])
    with np.errstate(all="ignore"):
        ok = np.all(np.abs(qf) < oref.Q_LIMIT, axis=1)
    q = np.where(ok[:, None], qf, 0).astype(np.int64)
    c, r = q >> 8, q & 255
    ok &= (c[:, 0] >= 0) & (c[:, 0] < prm["nx"]) & (c[:, 1] >= 0) & (c[:, 1] < prm["ny"]) & (c[:, 2] >= 0) & (c[:, 2] < prm["nz"])
    return ok, c, r


def cell_index(prm, c):
    return (c[:, 2] * prm["ny"] + c[:, 1]) * prm["nx"] + c[:, 0]


def moments(prm, pts, into=None):
    """dict(n uint32 [cells], S1 int64 [cells, 3], S2 int64 [cells, 6], used, ignored); into: a target to accumulate into"""
    nc = prm["nx"] * prm["ny"] * prm["nz"]
    T = into if into is not None else dict(n=np.zeros(nc, np.uint32), S1=np.zeros((nc, 3), np.int64), S2=np.zeros((nc, 6), np.int64))
    ok, c, r = voxel_of(prm, pts)
    cell, r = cell_index(prm, c[ok]), r[ok]
    np.add.at(T["n"], cell, 1)
    np.add.at(T["S1"], cell, r)
    np.add.at(T["S2"], cell, np.stack([r[:, a] * r[:, b] for a, b in S2_PAIRS], axis=1))
    T["used"], T["ignored"] = int(ok.sum()), int((~ok).sum())
    return T


def gaussians(prm, T):
    """mean [cells, 3], cov [cells, 6] (Sigma), icov [cells, 6] (Omega) in f64; zeros where n < min_points.  Adds them to T."""
    nc = len(T["n"])
    mean, cov, icov = np.zeros((nc, 3)), np.zeros((nc, 6)), np.zeros((nc, 6))
    res = float(F(prm["resolution"]))
    org = np.asarray(prm["origin"], F).astype(np.float64)
    u = res / 256.0
    u2 = u * u
    nx, ny = prm["nx"], prm["ny"]
    for cell in np.nonzero(T["n"] >= prm["min_points"])[0]:
        n = float(T["n"][cell])
        c = (cell % nx, (cell // nx) % ny, cell // (nx * ny))
        S1, S2 = T["S1"][cell].astype(np.float64), T["S2"][cell].astype(np.float64)
        for a in range(3):
            mean[cell, a] = (org[a] + res * c[a]) + u * ((S1[a] + 0.5 * n) / n)
        C = np.array([(u2 * (S2[k] - (S1[a] * S1[b]) / n)) / (n - 1.0) for k, (a, b) in enumerate(S2_PAIRS)])
        add = (prm["reg"] * ((C[0] + C[3]) + C[5])) / 3.0 + u2 / 12.0
        C[[0, 3, 5]] += add
        cov[cell] = C
        icov[cell] = cholesky_inverse(C)
    T.update(mean=mean, cov=cov, icov=icov)
    T["used_voxels"] = int((T["n"] >= prm["min_points"]).sum())
    T["sparse_voxels"] = int(((T["n"] > 0) & (T["n"] < prm["min_points"])).sum())
    return T


def cholesky_inverse(C):
    """Omega [6] of Sigma [6] (upper triangles 00 01 02 11 12 22): Sigma = L L^T column by column, Omega = L^-T L^-1"""
    l00 = math.sqrt(C[0])
    l10, l20 = C[1] / l00, C[2] / l00
    l11 = math.sqrt(C[3] - l10 * l10)
    l21 = (C[4] - l20 * l10) / l11
    l22 = math.sqrt((C[5] - l20 * l20) - l21 * l21)
    i00, i11, i22 = 1.0 / l00, 1.0 / l11, 1.0 / l22
    i10, i21 = -(l10 * i00) / l11, -(l21 * i11) / l22
    i20 = -(l20 * i00 + l21 * i10) / l22
    return np.array([(i00 * i00 + i10 * i10) + i20 * i20, i10 * i11 + i20 * i21, i20 * i22, i11 * i11 + i21 * i21, i21 * i22, i22 * i22])


def full3(u):
    return np.array([[u[0], u[1], u[2]], [u[1], u[3], u[4]], [u[2], u[4], u[5]]])


def build(prm, pts):
    return gaussians(prm, moments(prm, pts))


def add(prm, T, pts):
    return gaussians(prm, moments(prm, pts, into=T))


def stats(T):
    return [T["used"], T["ignored"], T["used_voxels"], T["sparse_voxels"]]


def evaluate(prm, T, src, pose, search=7, d2=D2_DEFAULT, reverse=False):
    """(acc [28]: the 21 of H, the 6 of g, S; n_in) at pose [7]"""
    p = np.asarray(src, F).reshape(-1, 3).astype(np.float64)
    if len(p) == 0:
        return np.zeros(28), 0
    R, t = gr.rot(pose[3:]), np.asarray(pose[:3], float)
    x = np.stack([((R[k, 0] * p[:, 0] + R[k, 1] * p[:, 1]) + R[k, 2] * p[:, 2]) + t[k] for k in range(3)], axis=1)
    qf = oref.quant_f(x.astype(F), prm["origin"], prm["resolution"])
    with np.errstate(all="ignore"):
        ok = np.all(np.abs(qf) < oref.Q_LIMIT, axis=1)
    c0 = np.where(ok[:, None], qf, 0).astype(np.int64) >> 8
    n = len(p)
    M, b, sw, any_ = np.zeros((n, 3, 3)), np.zeros((n, 3)), np.zeros(n), np.zeros(n, bool)
    hd = -0.5 * d2
    for s in range(search):
        c = c0 + OFFSETS[s]
        inside = ok & (c[:, 0] >= 0) & (c[:, 0] < prm["nx"]) & (c[:, 1] >= 0) & (c[:, 1] < prm["ny"]) & (c[:, 2] >= 0) & (c[:, 2] < prm["nz"])
        cell = np.where(inside, cell_index(prm, c), 0)
        O6 = T["icov"][cell]
        live = inside & (O6[:, 0] > 0.0)
        O = np.stack([O6[:, [0, 1, 2]], O6[:, [1, 3, 4]], O6[:, [2, 4, 5]]], axis=1)
        e = x - T["mean"][cell]
        Oe = np.stack([(O[:, k, 0] * e[:, 0] + O[:, k, 1] * e[:, 1]) + O[:, k, 2] * e[:, 2] for k in range(3)], axis=1)
        ss = (e[:, 0] * Oe[:, 0] + e[:, 1] * Oe[:, 1]) + e[:, 2] * Oe[:, 2]
        w = np.where(live, np.exp(hd * np.where(live, ss, 0.0)), 0.0)
        M = M + np.where(live[:, None, None], w[:, None, None] * O, 0.0)
        b = b + np.where(live[:, None], w[:, None] * Oe, 0.0)
        sw = sw + w
        any_ |= live
    P = np.zeros((n, 3, 3))
    P[:, 0, 1], P[:, 0, 2], P[:, 1, 0], P[:, 1, 2], P[:, 2, 0], P[:, 2, 1] = -p[:, 2], p[:, 1], p[:, 2], -p[:, 0], -p[:, 1], p[:, 0]
    A = -np.einsum("ij,njk->nik", R, P)
    J = np.concatenate([np.broadcast_to(np.eye(3), (n, 3, 3)), A], axis=2)   # [n, 3, 6]
    H = np.einsum("nka,nkl,nlb->nab", J, M, J)
    g = np.einsum("nka,nk->na", J, b)
    terms = np.concatenate([H[:, TRIU[0], TRIU[1]], g, sw[:, None]], axis=1)[any_]
    if reverse:
        terms = terms[::-1]
    acc = np.cumsum(terms, axis=0)[-1] if len(terms) else np.zeros(28)   # (one row after the other)
    return acc, int(any_.sum())


def solve(H21, g, lam):
    M = gr.info_full(H21)
    M = M + lam * np.diag(np.diag(M))
    return -(gr.block_inverse(M) @ g)


def accept(s_new, s_old):
    return s_new >= s_old - 64.0 * EPS * abs(s_old)


def align_one(prm, T, src, guess, reverse=False, **kw):
    """The loop of the header from one guess: dict(pose, score, info, n_in, status, accepted, rejected, last_step, lambda)"""
    a = dict(ALIGN, **kw)
    x = np.array(guess, float)
    acc, n_in = evaluate(prm, T, src, x, a["search"], a["d2"], reverse)
    out = dict(pose=x, score=0.0, info=np.zeros(21), n_in=0, status=NO_OVERLAP, accepted=0, rejected=0, last_step=0.0)
    out["lambda"] = a["lambda_init"]
    if n_in == 0:
        return out
    lam, cur, status, last = a["lambda_init"], acc, MAX_ITERATIONS, 0.0
    accepted = rejected = 0
    for _ in range(a["max_iterations"]):
        d = solve(cur[:21], cur[21:27], lam)
        step = float(np.max(np.abs(d))) if np.all(np.isfinite(d)) else math.inf
        xt = gr.retract(x, d) if math.isfinite(step) else x
        new, n_new = evaluate(prm, T, src, xt, a["search"], a["d2"], reverse)
        if math.isfinite(step) and accept(new[27], cur[27]):
            x, cur, n_in = xt, new, n_new
            accepted += 1
            last = step
            lam = max(lam / 3.0, a["lambda_min"])
            if step <= a["step_tol"]:
                status = CONVERGED
                break
        else:
            rejected += 1
            lam = min(4.0 * lam, a["lambda_max"])
    out.update(pose=x, score=float(cur[27]), info=cur[:21].copy(), n_in=n_in, status=status, accepted=accepted, rejected=rejected,
               last_step=last)
    out["lambda"] = lam
    return out


def best_of(results):
    b = (-1, -1)
    for k, r in enumerate(results):
        if r["status"] != NO_OVERLAP and (b[0] < 0 or r["score"] > results[b[0]]["score"]):
            b = (k, r["n_in"])
    return b


def align(prm, T, src, guesses, reverse=False, **kw):
    res = [align_one(prm, T, src, g, reverse, **kw) for g in guesses]
    return res, best_of(res)


def pose_distance(a, b):
    return gr.distance(np.asarray(a, float).reshape(1, 7), np.asarray(b, float).reshape(1, 7))
