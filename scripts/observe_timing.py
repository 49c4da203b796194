"""Timing of an aiding observation inside the 100 Hz cycle, on the bench scene (synth.make_scene(1 048 576, 65 536)).

One cycle is lv_filter_set (the posterior of a first LiDAR update: the running loop's state), 4 x lv_predict, ONE position fix,
lv_correct, lv_filter_get (the get ends in a wait for the device, so the host clock around the cycle is the cycle's wall time).  Three routes, alternated cycle by cycle in one process:
  `observe`   the fix through lv_observe (enqueue only, behind the queued predictions);
  `host`      what a user did before: lv_filter_get (launches the queued predictions and waits), the same rule in numpy
              (host_update below: H, S, Cholesky solve, gate, boxplus, Joseph form), lv_filter_set;
  `none`      the cycle without the fix, for scale (`passes`: the fix changes the prior, and with it the passes lv_correct takes).
`chain_*` are the same three without lv_correct (set, 4 x lv_predict, the fix, lv_filter_get): the fix's own cost, whatever the
LiDAR update makes of the moved prior.
Per route: `ms_median`, `ms_min`, `ms_p90` over --reps cycles after --warmup cycles of each route.  `host_numpy_ms_median` is the
numpy rule alone.  `routes_agree` is max |x_observe - x_host| and the same for P after one cycle from the same start (the two
routes round differently: 1e-9 is the project's chained bound).
`kernels` and `gap_us` come from a `rocprofv3 --kernel-trace --stats` run of its own (--profile-run: the observe route only),
attached afterwards: per kernel calls / average / min / max microseconds, and the gap between the end of the kernel in front of
observe_kernel (the predictions' launch) and its start.  Prints one JSON line; --out writes it too.

    python scripts/observe_timing.py --out plain.json
    rocprofv3 --kernel-trace --stats --output-format csv -d prof -o obs -- python scripts/observe_timing.py --profile-run
    python scripts/observe_timing.py --merge plain.json --stats prof/.../obs_kernel_stats.csv --trace prof/.../obs_kernel_trace.csv \
        --out profiles/observe_timing.json"""
import argparse
import csv
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

KERNELS = ("observe_kernel", "predict_kernel", "kf_to_filter_kernel")
S2_LEN = 98090.0 / 10000.0


# ---- the rule on the host, as a user of lv_filter_get / lv_filter_set writes it (position fix, all three components)
def _rot(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def _hat(v):
    return np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]])


def _exp(v):
    a = np.linalg.norm(v)
    s = 0.5 if a < 1e-8 else np.sin(a / 2) / a
    return np.r_[s * v, np.cos(a / 2)]


def _qmul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by + ay * bw + az * bx - ax * bz, aw * bz + az * bw + ax * by - ay * bx,
                     aw * bw - ax * bx - ay * by - az * bz])


def _boxplus(x, d):
    o = x.copy()
    o[0:3] += d[0:3]
    o[3:7] = _qmul(x[3:7], _exp(d[3:6]))
    o[7:11] = _qmul(x[7:11], _exp(d[6:9]))
    o[11:14] += d[9:12]
    o[14:17] += d[12:15]
    o[17:20] += d[15:18]
    o[20:23] += d[18:21]
    g = x[23:26]
    if g[0] + S2_LEN > 1e-11:   # the S2 chart of the filter (lv_manifold.hpp d_s2_Bx)
        r = 1.0 / (S2_LEN + g[0])
        B = np.array([[-g[1], -g[2]], [S2_LEN - g[1] * g[1] * r, -g[2] * g[1] * r], [-g[2] * g[1] * r, S2_LEN - g[2] * g[2] * r]]) / S2_LEN
    else:
        B = np.array([[0.0, 0.0], [0.0, -1.0], [1.0, 0.0]])
    o[23:26] = _rot(_exp(B @ d[21:23])) @ g
    return o


def host_update(x, P, z, Rm, lever, gate):
    Rw = _rot(x[3:7])
    H = np.zeros((3, 23))
    H[:, 0:3] = np.eye(3)
    H[:, 3:6] = -Rw @ _hat(lever)
    y = z - (x[0:3] + Rw @ lever)
    PHt = P @ H.T
    S = H @ PHt + Rm
    L = np.linalg.cholesky(S)
    w = np.linalg.solve(L, y)
    if gate > 0 and w @ w > gate:
        return x, P
    K = np.linalg.solve(S, PHt.T).T
    A = np.eye(23) - K @ H
    Pn = A @ P @ A.T + K @ Rm @ K.T
    return _boxplus(x, K @ y), (Pn + Pn.T) / 2


# ---- rocprofv3 output
def kernel_us(path):
    out = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            for key in KERNELS:
                if key in row["Name"]:
                    out[key] = dict(calls=int(row["Calls"]), avg_us=float(row["AverageNs"]) * 1e-3, min_us=float(row["MinNs"]) * 1e-3,
                                    max_us=float(row["MaxNs"]) * 1e-3)
    return out


def launch_gap_us(path):
    """Gaps between observe_kernel's start and the end of the kernel dispatched in front of it."""
    with open(path) as f:
        rows = list(csv.DictReader(f))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    gaps, before = [], {}
    for prev, cur in zip(rows, rows[1:]):
        if "observe_kernel" in cur["Kernel_Name"]:
            gaps.append((int(cur["Start_Timestamp"]) - int(prev["End_Timestamp"])) * 1e-3)
            name = next((k for k in KERNELS if k in prev["Kernel_Name"]), "other")
            before[name] = before.get(name, 0) + 1
    if not gaps:
        return None
    return dict(n=len(gaps), median=float(np.median(gaps)), min=float(np.min(gaps)), p90=float(np.percentile(gaps, 90)), kernel_in_front=before)


def merge(path, stats, trace, out):
    with open(path) as f:
        res = json.loads(f.readline())
    if stats:
        res["kernels"] = kernel_us(stats)
    if trace:
        res["gap_us"] = launch_gap_us(trace)
    line = json.dumps(res)
    print(line)
    if out:
        with open(out, "w") as f:
            f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=300, help="timed cycles per route")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--map-points", type=int, default=1_048_576)
    ap.add_argument("--scan-points", type=int, default=65_536)
    ap.add_argument("--profile-run", action="store_true", help="the observe route only, untimed (for a rocprofv3 run)")
    ap.add_argument("--merge", default=None, metavar="JSON", help="a result of this script to attach kernel times to (no GPU)")
    ap.add_argument("--stats", default=None, metavar="CSV", help="with --merge: rocprofv3's kernel_stats.csv")
    ap.add_argument("--trace", default=None, metavar="CSV", help="with --merge: rocprofv3's kernel_trace.csv")
    a = ap.parse_args()
    if a.merge:
        return merge(a.merge, a.stats, a.trace, a.out)
    import lvamd

    lvamd.load()
    from limo_velo_amd import aiding, capi, synth

    sc = synth.make_scene(a.map_points, a.scan_points)
    x0, P0 = sc["x_init"], sc["P0"]
    Q = np.diag([1e-4] * 3 + [1e-2] * 3 + [1e-5] * 3 + [1e-4] * 3)
    acc, gyro = np.array([0.0, 0.0, 9.809]), np.zeros(3)   # a static sensor: the map stays valid
    lever = np.array([0.3, -0.1, 0.45])
    z = sc["x_true"][0:3] + _rot(sc["x_true"][3:7]) @ lever
    Rm = np.eye(3) * 0.05 ** 2
    gate = aiding.chi2_gate(3, 0.999)
    fix = aiding.position(z, Rm, lever=lever, gate=gate)
    numpy_ms = []

    with capi.Context() as ctx:
        ctx.map_build(sc["map_xyz"])
        ctx.scan_set(sc["scan_xyz"])
        # every cycle starts from the posterior of a first LiDAR update, as the running loop does: from the scene's initial
        # covariance (1 rad^2 on attitude) a fix with a lever arm tilts the prior by degrees, and lv_correct then searches farther
        ctx.filter_set(x0, P0)
        ctx.correct(want_passes=False)
        x0, P0 = ctx.filter_get()

        def cycle(route):
            ctx.filter_set(x0, P0)
            for _ in range(4):
                ctx.predict(0.0025, Q, acc, gyro)
            if route == "observe":
                ctx.observe([fix])
            elif route == "host":
                x, P = ctx.filter_get()
                t0 = time.perf_counter()
                x, P = host_update(x, P, z, Rm, lever, gate)
                numpy_ms.append((time.perf_counter() - t0) * 1e3)
                ctx.filter_set(x, P)
            if not route_chain_only[0]:
                ctx.correct(want_passes=False)
            return ctx.filter_get()

        route_chain_only = [False]
        routes = ("observe",) if a.profile_run else ("observe", "host", "none")
        for _ in range(a.warmup):
            for r in routes:
                cycle(r)
        if a.profile_run:
            for _ in range(a.reps):
                cycle("observe")
            print(json.dumps(dict(profile_run=True, cycles=a.reps)))
            return
        numpy_ms.clear()
        ts = {r: [] for r in routes}
        for _ in range(a.reps):          # alternating: whatever else the host is doing hits the routes alike
            for r in routes:
                t0 = time.perf_counter()
                cycle(r)
                ts[r].append((time.perf_counter() - t0) * 1e3)
        passes = {}
        xo, Po = cycle("observe")
        passes["observe"] = ctx.last_passes()
        status = ctx.observe_results()[0]["status"]
        xh, Ph = cycle("host")
        passes["host"] = ctx.last_passes()
        xn, _ = cycle("none")
        passes["none"] = ctx.last_passes()
        route_chain_only[0] = True
        for _ in range(a.warmup):
            for r in routes:
                cycle(r)
        tc = {r: [] for r in routes}
        for _ in range(a.reps):
            for r in routes:
                t0 = time.perf_counter()
                cycle(r)
                tc[r].append((time.perf_counter() - t0) * 1e3)
    res = dict(what="set, 4 x lv_predict, one position fix, lv_correct, lv_filter_get", map_points=int(len(sc["map_xyz"])),
               scan_points=int(len(sc["scan_xyz"])), reps=a.reps, warmup=a.warmup, fix_status=int(status), routes={})
    for r in routes:
        t = np.array(ts[r])
        res["routes"][r] = dict(ms_median=float(np.median(t)), ms_min=float(t.min()), ms_p90=float(np.percentile(t, 90)), passes=int(passes[r]))
        t = np.array(tc[r])
        res["routes"]["chain_" + r] = dict(ms_median=float(np.median(t)), ms_min=float(t.min()), ms_p90=float(np.percentile(t, 90)))
    res["host_numpy_ms_median"] = float(np.median(numpy_ms))
    res["chain_observe_minus_none_ms"] = res["routes"]["chain_observe"]["ms_median"] - res["routes"]["chain_none"]["ms_median"]
    res["chain_host_minus_observe_ms"] = res["routes"]["chain_host"]["ms_median"] - res["routes"]["chain_observe"]["ms_median"]
    res["host_minus_observe_ms"] = res["routes"]["host"]["ms_median"] - res["routes"]["observe"]["ms_median"]
    res["routes_agree"] = dict(x=float(np.abs(xo - xh).max()), P=float(np.abs(Po - Ph).max()))
    res["fix_moved_the_result_m"] = float(np.abs(xo[:3] - xn[:3]).max())
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
