"""Timing of the rollouts (lv_occ_rollout) on the grid scripts/occupancy_timing.py builds: its ten 64 x 2048 sweeps integrated into
the default 512 x 512 x 64 grid at 0.2 m, a planar distance field over layers 18..24 (0.4 m .. 1.8 m above the ground), and a plan with
one goal about 20 m from the start (the cell nearest the first pose that has a metre of clearance; the goal is the first candidate
the start is reached from).  K = 8192 sequences of T = 64 steps of 0.1 s from the start, commands up to 2 m/s (0.2 m a
step: one cell) and 1.5 rad/s, with Tc = 1 (one constant command, DWA) and Tc = T (a full sequence, MPPI), and a footprint of 0, 16
and 64 points on the outline of a 0.8 m x 0.5 m robot.
  `ms`       host wall time of the whole call (upload of the controls, the kernel, the records and `best` copied back, the stream
             synchronised) after a warm-up call of every shape: median, 10th and 90th percentile of ROUNDS calls, the shapes of one
             footprint taken in turn within every round, so that they see the same machine;
  `kernel`   with --kernel-stats CSV (the kernel_stats.csv of a `rocprofv3 --kernel-trace --stats` run of this script with
             --profiled, which makes the Tc = T calls only): the rollout kernels' own times by group width;
  `steps`    good poses of all sequences together, `clear` sequences that reach T, `best` and `best_score`;
  `host`     what a caller without this call pays: `fetch_ms` (lv_occ_plan_fetch plus lv_occ_distance_fetch, median of 5) plus
             scripts/occ_rollout_host.cpp, the same rule (lv_rollout.hpp) built with g++ -O2 on one core, median of 3 runs.  Its
             steps, clear and best must equal the device's.
Prints one JSON line; --out writes it too.

    python scripts/occ_rollout_timing.py --sweeps /tmp/occ_sweeps.npz [--out profiles/occ_rollout_timing.json] [--kernel-stats CSV]"""
import argparse
import csv
import json
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import numpy as np  # noqa: E402

K, T, DT, ROUNDS = 8192, 64, 0.1, 400
VARIANTS = ["plain"]   # (the build measured under "staging_experiment" in the profile had "staged" beside it)


def spread(ts):
    return dict(median=float(np.median(ts)), p10=float(np.percentile(ts, 10)), p90=float(np.percentile(ts, 90)), n=len(ts))


def median_ms(fn, n):
    ts = []
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return spread(ts)


def in_turn(calls, rounds):
    """{name: spread} of the calls {name: fn}, each made once per round."""
    ts = {k: [] for k in calls}
    for _ in range(rounds):
        for k, fn in calls.items():
            t0 = time.perf_counter()
            fn()
            ts[k].append((time.perf_counter() - t0) * 1e3)
    return {k: spread(v) for k, v in ts.items()}


def kernel_ms(path):
    """{"G<g>": times} of the rollout kernels, by group width, from rocprofv3's kernel_stats.csv."""
    out = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            m = re.search(r"rollout_kernel<(\d+)>", row["Name"])
            if m:
                out[f"G{m.group(1)}"] = dict(
                    calls=int(row["Calls"]), avg_ms=float(row["AverageNs"]) * 1e-6, min_ms=float(row["MinNs"]) * 1e-6, max_ms=float(row["MaxNs"]) * 1e-6)
    return out


def outline(length, width, n):
    """n points round a rectangle's outline, evenly spaced along it."""
    t = (np.arange(n) + 0.5) / n * 4.0
    side, u = np.floor(t).astype(int), t - np.floor(t)
    hx, hy = 0.5 * length, 0.5 * width
    x = np.choose(side, [hx - 2 * hx * u, np.full(n, -hx), -hx + 2 * hx * u, np.full(n, hx)])
    y = np.choose(side, [np.full(n, hy), hy - 2 * hy * u, np.full(n, -hy), -hy + 2 * hy * u])
    return np.stack([x, y], axis=1).astype(np.float32)


def host_baseline(p, pot, cost, s2, jobs):
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "occ_rollout_host")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wno-unknown-pragmas", "-I" + os.path.join(ROOT, "tests", "emu"),
                               "-I" + os.path.join(ROOT, "limo-velo_amd", "csrc"), os.path.join(ROOT, "scripts", "occ_rollout_host.cpp"), "-o", exe])
        with open(os.path.join(d, "head"), "wb") as f:
            f.write(np.array(list(p.origin) + [p.resolution], np.float32).tobytes() + np.array([p.nx, p.ny], np.int32).tobytes())
        cost.tofile(os.path.join(d, "cost"))
        pot.tofile(os.path.join(d, "pot"))
        s2.tofile(os.path.join(d, "s2"))
        names = []
        for i, (prm, start, fp, u) in enumerate(jobs):
            names.append(os.path.join(d, f"job{i}"))
            with open(names[-1], "wb") as f:
                f.write(bytes(prm) + np.asarray(start, np.float32).tobytes() + np.array([len(fp), len(u)], np.int32).tobytes() + fp.tobytes() + u.tobytes())
        return json.loads(subprocess.check_output([exe] + [os.path.join(d, n) for n in ("head", "cost", "pot", "s2")] + names))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--sweeps", default=None)
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--profiled", action="store_true", help="the Tc = T calls only, 50 each, nothing written: the run to put under rocprofv3")
    a = ap.parse_args()
    import occupancy_timing

    sweeps, _ = occupancy_timing.make_sweeps(a.sweeps, count_visits=False)
    import lvamd

    lvamd.load()
    from limo_velo_amd import capi

    t0 = np.asarray(sweeps[0][1], np.float32)
    table = np.array([200, 100, 40, 15, 5, 1], np.uint8)
    rng = np.random.default_rng(5)
    res = dict(what="lv_occ_rollout", grid="512x512x64 @ 0.2 m (defaults), ten 64x2048 sweeps integrated; planar field over layers 18..24 (0.4 .. 1.8 m), one goal",
               batch=f"K = {K}, T = {T}, dt = {DT}", shapes=[])
    with capi.Context() as ctx:
        ctx.occ_configure()
        ctx.occ_integrate(sweeps)
        p = ctx.occ_params()
        ctx.occ_distance_build(capi.default_distance_params(planar=1, k_lo=18, k_hi=24))
        # the start: the cell nearest the first pose with a metre of clearance; the goal: such a cell about 20 m from it that the
        # plan reaches the start from
        s2, _ = ctx.occ_distance_fetch(metres=False)
        jj, ii = np.nonzero(s2 >= 25)
        xy = np.stack([p.origin[0] + (ii + 0.5) * p.resolution, p.origin[1] + (jj + 0.5) * p.resolution], axis=1)
        at = np.argmin(np.hypot(*(xy - t0[:2]).T))
        start = np.array([xy[at, 0], xy[at, 1], 0.0], np.float32)
        far = np.argsort(np.abs(np.hypot(*(xy - xy[at]).T) - 20.0))
        for g in far[::max(1, len(far) // 2000)][:40]:
            goal = np.array([[xy[g, 0], xy[g, 1], 0.0]], np.float32)
            stats = ctx.occ_plan_build(goal, table, capi.default_plan_params(connectivity=8, min_clear_s2=2))
            if ctx.occ_plan_fetch(cell_cost=False)[0][jj[at], ii[at]] != capi.LV_PLAN_UNREACHED:
                break
        else:
            raise SystemExit("no goal the start can be reached from")
        res["plan"] = dict(start=[float(v) for v in start], goal=[float(v) for v in goal[0]], goals_used=int(stats[0]), traversable=int(stats[1]),
                           reached=int(stats[2]))
        jobs, rows = [], []
        for n_fp in (0, 16, 64):
            fp = outline(0.8, 0.5, n_fp) if n_fp else np.zeros((0, 2), np.float32)
            calls, first = {}, {}
            for tc in (1, T):
                u = np.stack([rng.uniform(0.0, 2.0, (K, tc)), rng.uniform(-1.5, 1.5, (K, tc))], axis=-1).astype(np.float32)
                prm = capi.default_rollout_params(T=T, Tc=tc, dt=DT, fp_clear_s2=2, w_stop=20)
                jobs.append((prm, start, fp, u))
                for variant in VARIANTS:
                    def call(u=u, prm=prm, variant=variant):
                        return ctx.occ_rollout(start, u, prm, fp if len(fp) else None, ("results", "best"))

                    calls[(tc, variant)] = call
                    first[(tc, variant)] = call()   # warm-up: buffers, code objects
                assert all(first[(tc, v)][k].tobytes() == first[(tc, VARIANTS[0])][k].tobytes() for v in VARIANTS for k in ("results", "best"))
            if a.profiled:
                for _ in range(50):
                    for (tc, variant), fn in calls.items():
                        if tc == T:
                            fn()
                continue
            ms = in_turn(calls, ROUNDS)
            for tc in (1, T):
                out = first[(tc, VARIANTS[0])]
                rows.append(dict(Tc=tc, n_fp=n_fp, ms={v: ms[(tc, v)] for v in VARIANTS}, steps=int(out["results"]["steps"].sum()),
                                 clear=int((out["results"]["status"] == capi.LV_ROLLOUT_CLEAR).sum()), best=int(out["best"][0]),
                                 best_score=int(out["best"][1])))
                assert rows[-1]["steps"] > K and rows[-1]["best"] >= 0, rows[-1]
        if a.profiled:
            return
        fetch = median_ms(lambda: (ctx.occ_plan_fetch(), ctx.occ_distance_fetch(metres=False)), 5)
        pot, cost = ctx.occ_plan_fetch()
        s2, _ = ctx.occ_distance_fetch(metres=False)
    host = host_baseline(p, pot, cost, s2, jobs)
    for row, h in zip(rows, host):
        assert all(row[k] == h[k] for k in ("steps", "clear", "best", "best_score")), (row, h)
        row["host_ms"] = h["ms"]
    res["shapes"] = rows
    res["host_fetch_ms"] = fetch
    if a.kernel_stats:
        res["kernel_TcT"] = kernel_ms(a.kernel_stats)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
