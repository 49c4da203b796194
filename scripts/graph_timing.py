"""Timing of the pose-graph optimiser (lv_graph_set, lv_graph_optimise) on generated trajectories: 4096, 65536 and 2^18 keyframes
on laps of a 50 m circle (1024 keyframes a lap, with roll, pitch and height variation), odometry edges, 5 % loop edges between the
same place on different laps, a GPS prior (position only, lever arm) on every tenth keyframe, a start that drifts off the truth by a
random walk; with and without Huber (1.0 on every edge, 2 % of the loop edges false by 3 m).  Nothing is fixed: GPS holds the gauge.
Per case:
  `set_ms`        host wall time of lv_graph_set (copies and the incidence lists), median of --reps;
  `optimise_ms`   host wall time of lv_graph_optimise (step_tol 1e-6, at most 30 iterations), median of --reps, each after a fresh set;
  `iterations`, `pcg_iterations`, `ms_per_iteration`, `final_cost`, `status`  of that run (every repetition gives the same bits);
  `cpu`           the yardstick: the same Levenberg-Marquardt loop (same acceptance, lambda and stop rules) in numpy with
                  scipy.sparse assembly and scipy.sparse.linalg.spsolve as inner solver on one core: a DIFFERENT inner solver (a
                  direct factorisation, exact steps), so iterations differ; `final_cost` of both is given.  Sizes above --cpu-max
                  are not run on the CPU;
  `kernels`       calls and total ms per kernel from a `rocprofv3 --kernel-trace --stats` run of this script with --case NAME (one
                  optimise, no CPU yardstick), attached afterwards with --merge ... --attach NAME=kernel_stats.csv.
Prints one JSON line; --out writes it too.

    python scripts/graph_timing.py --out plain.json
    rocprofv3 --kernel-trace --stats --output-format csv -d prof -- python scripts/graph_timing.py --case n65536 --reps 1
    python scripts/graph_timing.py --merge plain.json --attach n65536=prof/.../kernel_stats.csv --out profiles/graph_timing.json"""
import argparse
import csv
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

LAP = 1024
SOLVE = dict(step_tol=1e-6, max_iterations=30)
EPS = 2.0 ** -52
EDGE_DTYPE = np.dtype([("i", "u4"), ("j", "u4"), ("t", "f8", 3), ("q", "f8", 4), ("info", "f8", 21), ("huber", "f8")])
PRIOR_DTYPE = np.dtype([("i", "u4"), ("reserved", "u4"), ("t", "f8", 3), ("q", "f8", 4), ("lever", "f8", 3), ("info", "f8", 21), ("huber", "f8")])
TRIU = np.triu_indices(6)
CASES = {f"n{n}{'_huber' if h else ''}": (n, h) for n in (4096, 65536, 1 << 18) for h in (False, True)}


# ---- batched algebra ([m, ...] arrays; the rule of include/limovelo_hip.h "Pose graph")
def rot(q):
    x, y, z, w = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    return np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w), 2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                     2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], axis=1).reshape(-1, 3, 3)


def qmul(a, b):
    ax, ay, az, aw = a.T
    bx, by, bz, bw = b.T
    return np.stack([aw * bx + ax * bw + ay * bz - az * by, aw * by + ay * bw + az * bx - ax * bz, aw * bz + az * bw + ax * by - ay * bx,
                     aw * bw - ax * bx - ay * by - az * bz], axis=1)


def qconj(a):
    return a * np.array([-1.0, -1.0, -1.0, 1.0])


def qlog(q):
    q = np.where(q[:, 3:4] < 0, -q, q)
    nv = np.linalg.norm(q[:, :3], axis=1)
    f = np.where(nv < 1e-12, 2.0 / q[:, 3], 2.0 * np.arctan2(nv, q[:, 3]) / np.maximum(nv, 1e-300))
    return f[:, None] * q[:, :3]


def qexp(v):
    th = np.linalg.norm(v, axis=1)
    f = np.where(th < 1e-8, 0.5 - th * th / 48.0, np.sin(0.5 * th) / np.maximum(th, 1e-300))
    return np.concatenate([f[:, None] * v, np.cos(0.5 * th)[:, None]], axis=1)


def hat(v):
    z = np.zeros(len(v))
    return np.stack([z, -v[:, 2], v[:, 1], v[:, 2], z, -v[:, 0], -v[:, 1], v[:, 0], z], axis=1).reshape(-1, 3, 3)


def jrinv(p):
    th2 = np.sum(p * p, axis=1)
    th = np.sqrt(th2)
    big = np.maximum(th, 1e-4)
    c = np.where(th < 1e-4, 1.0 / 12.0 + th2 / 720.0, 1.0 / (big * big) - (1.0 + np.cos(big)) / (2.0 * big * np.sin(big)))
    H = hat(p)
    return np.eye(3) + 0.5 * H + c[:, None, None] * (H @ H)


def info_full(u):
    W = np.zeros((len(u), 6, 6))
    W[:, TRIU[0], TRIU[1]] = u
    W[:, TRIU[1], TRIU[0]] = u
    return W


def huber(s, h):
    e = np.sqrt(s)
    out = (h > 0) & (e > h)
    safe = np.where(out, e, 1.0)
    return np.where(out, 2.0 * h * e - h * h, s), np.where(out, h / safe, 1.0)


def edge_res(x, E):
    xi, xj = x[E["i"]], x[E["j"]]
    Ri = rot(xi[:, 3:])
    dv = np.einsum("mba,mb->ma", Ri, xj[:, :3] - xi[:, :3])
    r = np.concatenate([dv - E["t"], qlog(qmul(qconj(E["q"]), qmul(qconj(xi[:, 3:]), xj[:, 3:])))], axis=1)
    return r, Ri, dv, xj


def prior_res(x, P):
    xi = x[P["i"]]
    Ri = rot(xi[:, 3:])
    r = np.concatenate([xi[:, :3] + np.einsum("mab,mb->ma", Ri, P["lever"]) - P["t"], qlog(qmul(qconj(P["q"]), xi[:, 3:]))], axis=1)
    return r, Ri


def cost_of(x, E, P, WE, WP):
    re, rp = edge_res(x, E)[0], prior_res(x, P)[0]
    se, sp = np.einsum("ma,mab,mb->m", re, WE, re), np.einsum("ma,mab,mb->m", rp, WP, rp)
    return 0.5 * (huber(se, E["huber"])[0].sum() + huber(sp, P["huber"])[0].sum())


def assemble(x, E, P, WE, WP):
    """(H csr [6n, 6n], g [6n], cost) with scipy.sparse"""
    import scipy.sparse as sp

    n = len(x)
    r, Ri, dv, xj = edge_res(x, E)
    s = np.einsum("ma,mab,mb->m", r, WE, r)
    rho, w = huber(s, E["huber"])
    J = jrinv(r[:, 3:])
    m = len(E)
    Ji, Jj = np.zeros((m, 6, 6)), np.zeros((m, 6, 6))
    RiT = np.transpose(Ri, (0, 2, 1))
    Ji[:, :3, :3], Ji[:, :3, 3:], Ji[:, 3:, 3:] = -RiT, hat(dv), -J @ np.transpose(rot(xj[:, 3:]), (0, 2, 1)) @ Ri
    Jj[:, :3, :3], Jj[:, 3:, 3:] = RiT, J
    W = w[:, None, None] * WE
    JiT, JjT = np.transpose(Ji, (0, 2, 1)), np.transpose(Jj, (0, 2, 1))
    rp, Rp = prior_res(x, P)
    spr = np.einsum("ma,mab,mb->m", rp, WP, rp)
    rhop, wp = huber(spr, P["huber"])
    Jp = np.zeros((len(P), 6, 6))
    Jp[:, :3, :3], Jp[:, :3, 3:], Jp[:, 3:, 3:] = np.eye(3), -Rp @ hat(P["lever"]), jrinv(rp[:, 3:])
    Wp = wp[:, None, None] * WP
    JpT = np.transpose(Jp, (0, 2, 1))
    blocks = [(E["i"], E["i"], JiT @ W @ Ji), (E["j"], E["j"], JjT @ W @ Jj), (E["i"], E["j"], JiT @ W @ Jj), (E["j"], E["i"], JjT @ W @ Ji),
              (P["i"], P["i"], JpT @ Wp @ Jp)]
    a6 = np.arange(6)
    rows = np.concatenate([(6 * bi.astype(np.int64)[:, None, None] + a6[None, :, None] + 0 * a6[None, None, :]).ravel() for bi, _, _ in blocks])
    cols = np.concatenate([(6 * bj.astype(np.int64)[:, None, None] + 0 * a6[None, :, None] + a6[None, None, :]).ravel() for _, bj, _ in blocks])
    vals = np.concatenate([b.ravel() for _, _, b in blocks])
    H = sp.coo_matrix((vals, (rows, cols)), shape=(6 * n, 6 * n)).tocsc()
    g = np.zeros((n, 6))
    np.add.at(g, E["i"], np.einsum("mab,mb->ma", JiT @ W, r))
    np.add.at(g, E["j"], np.einsum("mab,mb->ma", JjT @ W, r))
    np.add.at(g, P["i"], np.einsum("mab,mb->ma", JpT @ Wp, rp))
    return H, g.ravel(), 0.5 * (rho.sum() + rhop.sum())


def retract(x, d):
    d = d.reshape(-1, 6)
    q = qmul(x[:, 3:], qexp(d[:, 3:]))
    return np.concatenate([x[:, :3] + d[:, :3], q / np.linalg.norm(q, axis=1, keepdims=True)], axis=1)


def cpu_lm(x, E, P, prm):
    """The loop of the header with a direct inner solve"""
    import scipy.sparse as sp
    from scipy.sparse.linalg import spsolve

    WE, WP = info_full(E["info"]), info_full(P["info"])
    lam, acc, rej, status, fresh = prm["lambda_init"], 0, 0, 1, False
    for it in range(prm["max_iterations"]):
        if not fresh:
            H, g, c = assemble(x, E, P, WE, WP)
            if it == 0:
                cur = first = c
            fresh = True
        d = spsolve(H + lam * sp.diags(H.diagonal()), -g)
        xt = retract(x, d)
        cn = cost_of(xt, E, P, WE, WP)
        if cn <= cur + 64 * EPS * abs(cur):
            x, cur, fresh, acc = xt, cn, False, acc + 1
            lam = max(lam / 3.0, prm["lambda_min"])
            if np.max(np.abs(d)) <= prm["step_tol"]:
                status = 0
                break
        else:
            rej += 1
            lam = min(4.0 * lam, prm["lambda_max"])
    return x, dict(status=status, accepted=acc, rejected=rej, initial_cost=float(first), final_cost=float(cur))


# ---- the trajectories
def quat_rpy(roll, pitch, yaw):
    cr, sr, cp, sp_, cy, sy = np.cos(roll / 2), np.sin(roll / 2), np.cos(pitch / 2), np.sin(pitch / 2), np.cos(yaw / 2), np.sin(yaw / 2)
    return np.stack([sr * cp * cy - cr * sp_ * sy, cr * sp_ * cy + sr * cp * sy, cr * cp * sy - sr * sp_ * cy, cr * cp * cy + sr * sp_ * sy], axis=1)


def make_case(n, with_huber, seed=1):
    rng = np.random.default_rng(seed + n)
    a = 2 * np.pi * np.arange(n) / LAP
    truth = np.concatenate([np.stack([50 * np.cos(a), 50 * np.sin(a), 0.5 * np.sin(3 * a)], axis=1), quat_rpy(0.05 * np.sin(2 * a), 0.08 * np.cos(3 * a), a + np.pi / 2)], axis=1)
    n_loops = n // 20
    li = rng.integers(0, n - LAP, n_loops)
    lj = li + LAP * rng.integers(1, np.maximum((n - 1 - li) // LAP, 1) + 1)
    lj = np.minimum(lj, n - 1)
    keep = lj != li
    i, j = np.concatenate([np.arange(n - 1), li[keep]]), np.concatenate([np.arange(1, n), lj[keep]])
    st, sr = 0.02, 0.002
    E = np.zeros(len(i), EDGE_DTYPE)
    Ri = rot(truth[i, 3:])
    E["i"], E["j"] = i, j
    E["t"] = np.einsum("mba,mb->ma", Ri, truth[j, :3] - truth[i, :3]) + rng.normal(0, st, (len(i), 3))
    q = qmul(qmul(qconj(truth[i, 3:]), truth[j, 3:]), qexp(rng.normal(0, sr, (len(i), 3))))
    E["q"] = q / np.linalg.norm(q, axis=1, keepdims=True)
    E["info"] = np.diag([1 / st ** 2] * 3 + [1 / sr ** 2] * 3)[TRIU]
    if with_huber:
        E["huber"] = 1.0
        false = (n - 1) + rng.choice(len(i) - (n - 1), max(1, (len(i) - (n - 1)) // 50), replace=False)
        E["t"][false, 0] += 3.0
    lever = np.array([0.3, 0.1, 0.8])
    k = np.arange(0, n, 10)
    P = np.zeros(len(k), PRIOR_DTYPE)
    P["i"], P["lever"], P["q"] = k, lever, [0, 0, 0, 1]
    P["t"] = truth[k, :3] + np.einsum("mab,b->ma", rot(truth[k, 3:]), lever) + rng.normal(0, 1, (len(k), 3)) * np.array([0.2, 0.2, 0.5])
    Wg = np.zeros((6, 6))
    Wg[:3, :3] = np.diag([25.0, 25.0, 4.0])
    P["info"] = Wg[TRIU]
    start = truth.copy()
    start[:, :3] += np.cumsum(rng.normal(0, 0.005, (n, 3)), axis=0)
    yaw = np.cumsum(rng.normal(0, 0.0002, n))
    sq = qmul(truth[:, 3:], qexp(np.stack([0 * yaw, 0 * yaw, yaw], axis=1)))
    start[:, 3:] = sq / np.linalg.norm(sq, axis=1, keepdims=True)
    return start, E, P, truth


def spread(ts):
    return dict(median=float(np.median(ts)), min=float(np.min(ts)), max=float(np.max(ts)), n=len(ts))


def kernel_ms(path):
    out = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            if "graph_" in row["Name"] or "pcg_" in row["Name"]:
                name = row["Name"].replace("(anonymous namespace)::", "").replace("void ", "").replace("lv::", "").split("(")[0]
                out[name] = dict(calls=int(row["Calls"]), total_ms=float(row["TotalDurationNs"]) * 1e-6, avg_us=float(row["AverageNs"]) * 1e-3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--case", default=None, choices=sorted(CASES), help="this case only, no CPU yardstick (for a profiled run)")
    ap.add_argument("--merge", default=None)
    ap.add_argument("--attach", action="append", default=None, metavar="CASE=CSV")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cpu-max", type=int, default=65536)
    ap.add_argument("--cpu-only", action="store_true", help="the yardstick alone (no GPU needed)")
    a = ap.parse_args()
    if a.merge:
        with open(a.merge) as f:
            res = json.loads(f.readline())
        for item in a.attach or []:
            name, path = item.split("=", 1)
            ks = kernel_ms(path)
            res["cases"][name]["kernels"] = ks
            res["cases"][name]["kernels_ms_sum"] = sum(v["total_ms"] for v in ks.values())
    else:
        res = dict(what="lv_graph_set / lv_graph_optimise", solve=SOLVE, reps=a.reps, cases={})
        ctx = None
        if not a.cpu_only:
            import lvamd

            lvamd.load()
            from limo_velo_amd import capi

            ctx = capi.Context()
        for name, (n, h) in CASES.items():
            if a.case and name != a.case:
                continue
            start, E, P, truth = make_case(n, h)
            row = dict(n=n, n_edges=len(E), n_priors=len(P), huber=h)
            if ctx is not None:
                ctx.graph_set(start, None, E, P)
                ctx.graph_optimise(**SOLVE)   # warm-up: allocation, code objects
                ts, to = [], []
                for _ in range(a.reps):
                    t0 = time.perf_counter()
                    ctx.graph_set(start, None, E, P)
                    t1 = time.perf_counter()
                    info = ctx.graph_optimise(**SOLVE)
                    t2 = time.perf_counter()
                    ts.append((t1 - t0) * 1e3)
                    to.append((t2 - t1) * 1e3)
                its = info["accepted"] + info["rejected"]
                x = ctx.graph_fetch()
                row.update(set_ms=spread(ts), optimise_ms=spread(to), iterations=its, accepted=info["accepted"], pcg_iterations=info["pcg_iterations"],
                           ms_per_iteration=float(np.median(to)) / max(its, 1), status=info["status"], initial_cost=info["initial_cost"],
                           final_cost=info["final_cost"], longest_list=info["longest_list"],
                           position_error_m=dict(start=float(np.linalg.norm(start[:, :3] - truth[:, :3], axis=1).max()),
                                                 end=float(np.linalg.norm(x[:, :3] - truth[:, :3], axis=1).max())))
            if (not a.case or a.cpu_only) and n <= a.cpu_max:
                t0 = time.perf_counter()
                xc, ci = cpu_lm(start, E, P, dict(lambda_init=1e-4, lambda_min=1e-10, lambda_max=1e8, **SOLVE))
                ms = (time.perf_counter() - t0) * 1e3
                row["cpu"] = dict(ms=ms, method="numpy + scipy.sparse assembly, scipy.sparse.linalg.spsolve, one core", **ci,
                                  ms_per_iteration=ms / max(ci["accepted"] + ci["rejected"], 1))
                if "optimise_ms" in row:
                    row["cpu_over_device"] = ms / row["optimise_ms"]["median"]
                    row["final_cost_relative_difference"] = abs(row["final_cost"] - ci["final_cost"]) / ci["final_cost"]
            res["cases"][name] = row
            print(json.dumps({name: row}), file=sys.stderr)
        if ctx is not None:
            ctx.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
