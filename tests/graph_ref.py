"""The pose-graph rule of include/limovelo_hip.h "Pose graph" restated in numpy f64 (TEST INFRASTRUCTURE): residuals, Jacobians,
cost and retraction, a dense Gauss-Newton solver, the Levenberg-Marquardt loop with a dense or a conjugate-gradient inner solve, and a
seeded generator of graphs.  tests/test_graph_ref.py checks it against itself (central differences, LM against dense Gauss-Newton);
the host build of lv_graph.hpp and the device are held to it."""
import math

import numpy as np

EPS = 2.0 ** -52
POSE_DTYPE = np.dtype([("t", "f8", 3), ("q", "f8", 4)])
EDGE_DTYPE = np.dtype([("i", "u4"), ("j", "u4"), ("t", "f8", 3), ("q", "f8", 4), ("info", "f8", 21), ("huber", "f8")])
PRIOR_DTYPE = np.dtype([("i", "u4"), ("reserved", "u4"), ("t", "f8", 3), ("q", "f8", 4), ("lever", "f8", 3), ("info", "f8", 21), ("huber", "f8")])
assert POSE_DTYPE.itemsize == 56 and EDGE_DTYPE.itemsize == 240 and PRIOR_DTYPE.itemsize == 264
TRIU = np.triu_indices(6)
DEFAULTS = dict(max_iterations=100, pcg_max_iterations=1000, pcg_tol=1e-2, step_tol=1e-8, lambda_init=1e-4, lambda_min=1e-10, lambda_max=1e8)
CONVERGED, MAX_ITERATIONS = 0, 1
SERIES_TH = 1e-4


# ---- algebra
def hat(v):
    return np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])


def rot(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def qmul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by + ay * bw + az * bx - ax * bz, aw * bz + az * bw + ax * by - ay * bx,
                     aw * bw - ax * bx - ay * by - az * bz])


def qconj(a):
    return np.array([-a[0], -a[1], -a[2], a[3]])


def qlog(q):
    q = np.asarray(q, float)
    if q[3] < 0:
        q = -q
    nv = math.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2])
    f = 2.0 / q[3] if nv < 1e-12 else 2.0 * math.atan2(nv, q[3]) / nv
    return f * q[:3]


def qexp(v):
    v = np.asarray(v, float)
    th = math.sqrt(v @ v)
    f = 0.5 - th * th / 48.0 if th < 1e-8 else math.sin(0.5 * th) / th
    return np.array([f * v[0], f * v[1], f * v[2], math.cos(0.5 * th)])


def jrinv(p):
    th2 = float(p @ p)
    th = math.sqrt(th2)
    c = 1.0 / 12.0 + th2 / 720.0 if th < SERIES_TH else 1.0 / th2 - (1.0 + math.cos(th)) / (2.0 * th * math.sin(th))
    H = hat(p)
    return np.eye(3) + 0.5 * H + c * (H @ H)


def info_full(u):
    W = np.zeros((6, 6))
    W[TRIU] = u
    return W + np.triu(W, 1).T


def info21(M):
    return np.asarray(M, float)[TRIU]


def rho_w(s, huber):
    if not huber > 0:
        return s, 1.0
    e = math.sqrt(s)
    if e <= huber:
        return s, 1.0
    return 2.0 * huber * e - huber * huber, huber / e


def retract(x, d):
    """x [7] (t, q), d [6] -> [7]"""
    q = qmul(x[3:], qexp(d[3:]))
    return np.concatenate([x[:3] + d[:3], q / math.sqrt(q @ q)])


def retract_all(x, d, fixed):
    out = x.copy()
    for k in range(len(x)):
        if not fixed[k]:
            out[k] = retract(x[k], d[6 * k:6 * k + 6])
    return out


# ---- factors
def edge_residual(xi, xj, e):
    Ri = rot(xi[3:])
    r = np.empty(6)
    r[:3] = Ri.T @ (xj[:3] - xi[:3]) - e["t"]
    r[3:] = qlog(qmul(qconj(e["q"]), qmul(qconj(xi[3:]), xj[3:])))
    return r


def edge_jacobians(xi, xj, r):
    Ri, Rj = rot(xi[3:]), rot(xj[3:])
    dv = Ri.T @ (xj[:3] - xi[:3])
    J = jrinv(r[3:])
    Ji, Jj = np.zeros((6, 6)), np.zeros((6, 6))
    Ji[:3, :3] = -Ri.T
    Ji[:3, 3:] = hat(dv)
    Ji[3:, 3:] = -J @ Rj.T @ Ri
    Jj[:3, :3] = Ri.T
    Jj[3:, 3:] = J
    return Ji, Jj


def prior_residual(xi, p):
    Ri = rot(xi[3:])
    r = np.empty(6)
    r[:3] = xi[:3] + Ri @ p["lever"] - p["t"]
    r[3:] = qlog(qmul(qconj(p["q"]), xi[3:]))
    return r


def prior_jacobian(xi, p, r):
    Ri = rot(xi[3:])
    Ji = np.zeros((6, 6))
    Ji[:3, :3] = np.eye(3)
    Ji[:3, 3:] = -Ri @ hat(p["lever"])
    Ji[3:, 3:] = jrinv(r[3:])
    return Ji


def edge_lin(xi, xj, e):
    """r, s, w, rho, Hii, Hjj, Hij, gi, gj of one edge"""
    r = edge_residual(xi, xj, e)
    W = info_full(e["info"])
    s = float(r @ W @ r)
    rho, w = rho_w(s, float(e["huber"]))
    Ji, Jj = edge_jacobians(xi, xj, r)
    W = w * W
    return dict(r=r, s=s, w=w, rho=rho, Hii=Ji.T @ W @ Ji, Hjj=Jj.T @ W @ Jj, Hij=Ji.T @ W @ Jj, gi=Ji.T @ W @ r, gj=Jj.T @ W @ r)


def prior_lin(xi, p):
    r = prior_residual(xi, p)
    W = info_full(p["info"])
    s = float(r @ W @ r)
    rho, w = rho_w(s, float(p["huber"]))
    Ji = prior_jacobian(xi, p, r)
    W = w * W
    return dict(r=r, s=s, w=w, rho=rho, Hii=Ji.T @ W @ Ji, gi=Ji.T @ W @ r)


# ---- a graph: dict(poses [n, 7], fixed [n] bool, edges EDGE_DTYPE, priors PRIOR_DTYPE)
def make_graph(poses, fixed=None, edges=None, priors=None):
    poses = np.ascontiguousarray(poses, float)
    n = len(poses)
    return dict(poses=poses, fixed=np.zeros(n, bool) if fixed is None else np.asarray(fixed, bool),
                edges=np.zeros(0, EDGE_DTYPE) if edges is None else np.asarray(edges, EDGE_DTYPE),
                priors=np.zeros(0, PRIOR_DTYPE) if priors is None else np.asarray(priors, PRIOR_DTYPE))


def edge_record(i, j, t, q, info, huber=0.0):
    e = np.zeros((), EDGE_DTYPE)
    e["i"], e["j"], e["t"], e["q"], e["info"], e["huber"] = i, j, t, q, info21(info), huber
    return e


def prior_record(i, t, q, lever, info, huber=0.0):
    p = np.zeros((), PRIOR_DTYPE)
    p["i"], p["t"], p["q"], p["lever"], p["info"], p["huber"] = i, t, q, lever, info21(info), huber
    return p


def chi2(g, x):
    es = np.array([rho_s(edge_residual(x[e["i"]], x[e["j"]], e), e)[0] for e in g["edges"]])
    ps = np.array([rho_s(prior_residual(x[p["i"]], p), p)[0] for p in g["priors"]])
    return es, ps


def rho_s(r, f):
    s = float(r @ info_full(f["info"]) @ r)
    return s, rho_w(s, float(f["huber"]))[0]


def cost(g, x):
    c = 0.0
    for e in g["edges"]:
        c += rho_s(edge_residual(x[e["i"]], x[e["j"]], e), e)[1]
    for p in g["priors"]:
        c += rho_s(prior_residual(x[p["i"]], p), p)[1]
    return 0.5 * c


def linearise(g, x):
    """dense H [6n, 6n], g [6n] (rows and columns of fixed nodes zero), cost"""
    n = len(x)
    H, b, c = np.zeros((6 * n, 6 * n)), np.zeros(6 * n), 0.0
    for e in g["edges"]:
        i, j = int(e["i"]), int(e["j"])
        L = edge_lin(x[i], x[j], e)
        si, sj = slice(6 * i, 6 * i + 6), slice(6 * j, 6 * j + 6)
        H[si, si] += L["Hii"]
        H[sj, sj] += L["Hjj"]
        H[si, sj] += L["Hij"]
        H[sj, si] += L["Hij"].T
        b[si] += L["gi"]
        b[sj] += L["gj"]
        c += L["rho"]
    for p in g["priors"]:
        i = int(p["i"])
        L = prior_lin(x[i], p)
        si = slice(6 * i, 6 * i + 6)
        H[si, si] += L["Hii"]
        b[si] += L["gi"]
        c += L["rho"]
    dead = np.repeat(g["fixed"], 6)
    H[dead, :] = 0.0
    H[:, dead] = 0.0
    b[dead] = 0.0
    return H, b, 0.5 * c


def block_inverse(M):
    """The Cholesky inverse of lv_graph.hpp: a pivot that is not positive gives that component a zero row and column."""
    L, Li, live = np.zeros((6, 6)), np.zeros((6, 6)), [False] * 6
    for k in range(6):
        d = M[k, k] - sum(L[k, m] * L[k, m] for m in range(k))
        live[k] = bool(d > 0.0 and d < math.inf)
        if not live[k]:
            continue
        L[k, k] = math.sqrt(d)
        for a in range(k + 1, 6):
            L[a, k] = (M[a, k] - sum(L[a, m] * L[k, m] for m in range(k))) / L[k, k]
    for c in range(6):
        if not live[c]:
            continue
        Li[c, c] = 1.0 / L[c, c]
        for a in range(c + 1, 6):
            if live[a]:
                Li[a, c] = -sum(L[a, m] * Li[m, c] for m in range(c, a)) / L[a, a]
    return Li.T @ Li


def pcg(A, b, fixed, tol, max_iterations):
    """(d, iterations) of A d = -b from d = 0, preconditioned by the inverse 6 x 6 diagonal blocks"""
    n = len(fixed)
    Minv = np.zeros_like(A)
    for k in range(n):
        if not fixed[k]:
            s = slice(6 * k, 6 * k + 6)
            Minv[s, s] = block_inverse(A[s, s])
    d = np.zeros_like(b)
    r = -b
    z = Minv @ r
    p = z.copy()
    rz = rz0 = float(r @ z)
    if not (rz0 > 0 and rz0 < math.inf):
        return d, 0
    its = 0
    for _ in range(max_iterations):
        Ap = A @ p
        pAp = float(p @ Ap)
        if not (pAp > 0 and pAp < math.inf):
            break
        alpha = rz / pAp
        d += alpha * p
        r -= alpha * Ap
        z = Minv @ r
        rzn = float(r @ z)
        its += 1
        if not rzn > tol * tol * rz0 or not rzn < math.inf:
            break
        p = z + (rzn / rz) * p
        rz = rzn
    return d, its


def accept(cost_new, cost_old):
    return cost_new <= cost_old + 64.0 * EPS * abs(cost_old)


def lm(g, x0=None, inner="pcg", **kw):
    """The loop of the header.  Returns (poses, info): info has status, accepted, rejected, pcg_iterations, initial_cost,
    final_cost, last_step, lambda and costs (after every accepted step)."""
    prm = dict(DEFAULTS, **kw)
    x = np.array(g["poses"] if x0 is None else x0, float)
    fixed = g["fixed"]
    free = ~np.repeat(fixed, 6)
    lam = prm["lambda_init"]
    info = dict(status=MAX_ITERATIONS, accepted=0, rejected=0, pcg_iterations=0, last_step=0.0, costs=[])
    fresh = False
    for it in range(prm["max_iterations"]):
        if not fresh:
            H, b, c = linearise(g, x)
            if it == 0:
                cur = info["initial_cost"] = c
            fresh = True
        A = H + lam * np.diag(np.diag(H))
        if inner == "pcg":
            d, its = pcg(A, b, fixed, prm["pcg_tol"], prm["pcg_max_iterations"])
            info["pcg_iterations"] += its
        else:
            d = np.zeros_like(b)
            d[free] = np.linalg.solve(A[np.ix_(free, free)], -b[free])
        xt = retract_all(x, d, fixed)
        cn = cost(g, xt)
        step = float(np.max(np.abs(d)))
        if math.isfinite(step) and accept(cn, cur):
            x, cur, fresh = xt, cn, False
            info["accepted"] += 1
            info["last_step"] = step
            info["costs"].append(cn)
            lam = max(lam / 3.0, prm["lambda_min"])
            if step <= prm["step_tol"]:
                info["status"] = CONVERGED
                break
        else:
            info["rejected"] += 1
            lam = min(4.0 * lam, prm["lambda_max"])
    info["final_cost"] = cur
    info["lambda"] = lam
    return x, info


def dense_gn(g, x0=None, iterations=300, tol=1e-13):
    """Gauss-Newton with dense solves from x0; a step that raises the cost is halved (up to 30 times).  Returns (poses, cost)."""
    x = np.array(g["poses"] if x0 is None else x0, float)
    fixed = g["fixed"]
    free = ~np.repeat(fixed, 6)
    for _ in range(iterations):
        H, b, c = linearise(g, x)
        d = np.zeros_like(b)
        d[free] = np.linalg.solve(H[np.ix_(free, free)], -b[free])
        f = 1.0
        for _ in range(30):
            xt = retract_all(x, f * d, fixed)
            if accept(cost(g, xt), c):
                break
            f *= 0.5
        x = xt
        if f * np.max(np.abs(d)) < tol:
            break
    return x, cost(g, x)


def distance(a, b):
    """max over nodes of |dt| and |Log(Ra^T Rb)|"""
    dt = np.max(np.linalg.norm(a[:, :3] - b[:, :3], axis=1))
    dr = max(float(np.linalg.norm(qlog(qmul(qconj(p[3:]), q[3:])))) for p, q in zip(a, b))
    return max(float(dt), dr)


# ---- the generator
def quat_rpy(roll, pitch, yaw):
    cr, sr, cp, sp, cy, sy = math.cos(roll / 2), math.sin(roll / 2), math.cos(pitch / 2), math.sin(pitch / 2), math.cos(yaw / 2), math.sin(yaw / 2)
    return np.array([sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy, cr * cp * cy + sr * sp * sy])


def relative(a, b):
    """T_a^-1 T_b as (t [3], q [4]) of two poses [7]"""
    return rot(a[3:]).T @ (b[:3] - a[:3]), qmul(qconj(a[3:]), b[3:])


def compose(a, t, q):
    qq = qmul(a[3:], q)
    return np.concatenate([a[:3] + rot(a[3:]) @ t, qq / math.sqrt(qq @ qq)])


def circle(n, radius=10.0):
    """n true poses on a circle, heading along it, with roll, pitch and height variation"""
    out = np.zeros((n, 7))
    for k in range(n):
        a = 2 * math.pi * k / n
        out[k, :3] = radius * math.cos(a), radius * math.sin(a), 0.5 * math.sin(3 * a)
        out[k, 3:] = quat_rpy(0.05 * math.sin(2 * a), 0.08 * math.cos(3 * a), a + math.pi / 2)
    return out


def random_info(rng, sigma_t, sigma_r, spread=0.1):
    """diag(1 / sigma^2) with a dense random perturbation; symmetric positive definite"""
    L = np.diag([1 / sigma_t] * 3 + [1 / sigma_r] * 3) @ (np.eye(6) + spread * rng.normal(size=(6, 6)))
    return L.T @ L


def ring(n, seed, loops=0, noise=True, sigma_t=0.02, sigma_r=0.004, drift=(0.01, 0.002), huber=0.0, ring_closed=True):
    """(graph with a dead-reckoned, drifted start and nothing fixed yet, true poses).  Odometry edges k -> k + 1 (and n - 1 -> 0 when
    ring_closed), `loops` random loop edges, every measurement the true relative pose moved by noise of (sigma_t, sigma_r)."""
    rng = np.random.default_rng(seed)
    truth = circle(n)

    def measure(i, j):
        t, q = relative(truth[i], truth[j])
        if noise:
            t = t + rng.normal(0, sigma_t, 3)
            q = qmul(q, qexp(rng.normal(0, sigma_r, 3)))
        return edge_record(i, j, t, q / math.sqrt(q @ q), random_info(rng, sigma_t, sigma_r), huber)

    edges = [measure(k, k + 1) for k in range(n - 1)]
    start = [truth[0].copy()]
    for k in range(n - 1):   # dead reckoning with a drift on top of the odometry
        e = edges[k]
        start.append(compose(start[-1], e["t"] + np.array([drift[0], 0, 0]), qmul(e["q"], qexp([0, 0, drift[1]]))))
    if ring_closed and n > 2:
        edges.append(measure(n - 1, 0))
    for _ in range(loops):
        i, j = rng.choice(n, 2, replace=False)
        edges.append(measure(int(i), int(j)))
    return make_graph(np.array(start), None, np.array(edges, EDGE_DTYPE)), truth


def gps_priors(truth, nodes, lever=(0.3, 0.1, 0.8), sigma=(0.2, 0.2, 0.5), rng=None, huber=0.0):
    """Position-only priors: the antenna at t + R lever, rotation rows and columns of info zero"""
    out = []
    for k in nodes:
        z = truth[k, :3] + rot(truth[k, 3:]) @ np.asarray(lever)
        if rng is not None:
            z = z + rng.normal(0, 1, 3) * np.asarray(sigma)
        W = np.zeros((6, 6))
        W[:3, :3] = np.diag(1.0 / np.asarray(sigma) ** 2)
        out.append(prior_record(k, z, [0, 0, 0, 1], lever, W, huber))
    return np.array(out, PRIOR_DTYPE)
