"""Timing of the lattice planner (lv_occ_lattice_build, lv_occ_lattice_paths) over the default 512 x 512 x 64 grid at 0.2 m after the
ten sweeps of scripts/occupancy_timing.py: a planar plan over a band of six layers that starts two layers above the ground (as
scripts/occ_plan_timing.py's `planar_above_ground`), one goal, H = 16, and two tables from limo_velo_amd.lattice.primitives: one of
reach 2 (min_radius 0: the lattice vectors and the shortest turns) and one of reach 8 (the largest min_radius whose table fits).
Per table:
  `build_ms`      host wall time of lv_occ_lattice_build (copies, seed, the rounds with their read-backs, stats): median, p10, p90
                  over --reps calls after two warm-up calls;
  `rounds`, `tile`, `reach`  as lv_occ_lattice_info reports them (measured);
  `kernel_launches_derived`, `read_backs_derived`  NOT measured: worked out from `rounds` (batches of PLAN_ROUNDS_PER_READ = 8
                  launches between two reads of the round words, plus the seed and stats kernels);
  `paths`         for 1, 1024 and 65536 random starts with random headings: median wall time of lv_occ_lattice_paths and the number
                  of path states returned;
  `host`          the first yardstick, what a caller without the lattice pays: `fetch_ms` (lv_occ_plan_fetch of the cost bytes,
                  median of 5) plus scripts/occ_lattice_host.cpp, the same rule as a Dijkstra with a binary heap, g++ -O2, one
                  core (`solve_ms`, median of 3 runs).  Its V must equal the device's on every state: asserted.
  `vs_host`       (fetch_ms + solve_ms) / build_ms median;
  `vs_plan_build` build_ms median / the median of lv_occ_plan_build on the same field: the second yardstick, the holonomic build
                  at 1/16 of the states.
Prints one JSON line; --out writes it too.

    python scripts/occ_lattice_timing.py --sweeps /tmp/occ_sweeps.npz --out profiles/occ_lattice_timing.json"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402

ROUNDS_PER_READ = 8
H = 16
N_STARTS = (1, 1024, 65536)
ROBOT_RADIUS, INFLATION_RADIUS = 0.3, 1.0


def spread(ts):
    return dict(median=float(np.median(ts)), p10=float(np.percentile(ts, 10)), p90=float(np.percentile(ts, 90)), n=len(ts))


def reach_of(t):
    r = t[t["length"] != 0]
    sw = np.abs(r["sweep"].astype(np.int64)).max(initial=0)
    return int(max(np.abs(r["di"].astype(np.int64)).max(initial=0), np.abs(r["dj"].astype(np.int64)).max(initial=0), sw))


def tables(lattice, res):
    """{name: (min_radius, table)}: reach 2, and the widest table the generator makes on this grid."""
    out = {"reach2": (0.0, lattice.primitives(H, 0.0, res))}
    best = None
    for k in range(1, 200):
        try:
            t = lattice.primitives(H, 0.05 * k, res)
        except ValueError:
            continue
        if best is None or reach_of(t) >= reach_of(best[1]):
            best = (0.05 * k, t)
    out["reach8"] = best
    return out


def host_solve(cost, t, goal_states):
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "occ_lattice_host")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wno-unknown-pragmas", "-I" + os.path.join(ROOT, "tests", "emu"),
                               "-I" + os.path.join(ROOT, "limo-velo_amd", "csrc"), os.path.join(ROOT, "scripts", "occ_lattice_host.cpp"), "-o", exe])
        ny, nx = cost.shape
        np.array([nx, ny, t.shape[0], t.shape[1], len(goal_states)], np.int32).tofile(os.path.join(d, "head"))
        np.ascontiguousarray(cost, np.uint8).tofile(os.path.join(d, "cost"))
        np.ascontiguousarray(t).tofile(os.path.join(d, "prims"))
        np.asarray(goal_states, np.int32).tofile(os.path.join(d, "goals"))
        ms = []
        for _ in range(3):
            out = subprocess.run([exe] + [os.path.join(d, n) for n in ("head", "cost", "prims", "goals", "V")], stdout=subprocess.PIPE, check=True, timeout=600)
            ms.append(float(out.stdout.decode().split()[-1]))
        return float(np.median(ms)), np.fromfile(os.path.join(d, "V"), np.uint32).reshape(t.shape[0], ny, nx)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--sweeps", default=None)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    import occupancy_timing

    views, _ = occupancy_timing.make_sweeps(a.sweeps, count_visits=False)
    import lvamd

    lvamd.load()
    from limo_velo_amd import capi, lattice, occupancy

    rng = np.random.default_rng(1)
    res_out = dict(what="lv_occ_lattice_build / lv_occ_lattice_paths", grid="512x512x64 @ 0.2 m (defaults)", H=H, reps=a.reps,
                   rounds_per_read=ROUNDS_PER_READ, tables={})
    with capi.Context() as ctx:
        ctx.occ_configure()
        ctx.occ_integrate(views)
        p = ctx.occ_params()
        res = float(p.resolution)
        L = ctx.occ_fetch()
        ground = int(np.argmax(np.sum(L >= np.float32(p.l_occ), axis=(1, 2))))
        del L
        dist = dict(planar=1, k_lo=ground + 2, k_hi=ground + 7)
        ctx.occ_distance_build(capi.default_distance_params(**dist))
        table = occupancy.inflation_cost_table(res, ROBOT_RADIUS, INFLATION_RADIUS)
        pp = capi.default_plan_params(connectivity=8, min_clear_s2=occupancy.min_clear_s2(res, ROBOT_RADIUS))
        s2, _ = ctx.occ_distance_fetch(metres=False)
        at = np.argwhere((s2 >= int(pp.min_clear_s2)) & (s2 < capi.LV_OCC_FAR))
        j, i = at[np.argmin(((at - np.array(s2.shape) // 2) ** 2).sum(axis=1))]
        goal = np.array([[p.origin[0] + (i + 0.5) * res, p.origin[1] + (j + 0.5) * res, 0.0]], np.float32)
        for _ in range(2):
            ctx.occ_plan_build(goal, table, pp)
        ts = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            ctx.occ_plan_build(goal, table, pp)
            ts.append((time.perf_counter() - t0) * 1e3)
        info = ctx.occ_plan_info()
        res_out.update(distance=dist, goal_cell=[int(i), int(j)], plan_build_ms=spread(ts), plan_rounds=int(info.rounds), field=[info.nx, info.ny])
        ts = []
        for _ in range(5):
            t0 = time.perf_counter()
            _, cost = ctx.occ_plan_fetch(potential=False)
            ts.append((time.perf_counter() - t0) * 1e3)
        fetch_ms = float(np.median(ts))
        goals = np.zeros(1, capi.LATTICE_POSE_DTYPE)
        goals["xyz"], goals["h"] = goal, 0
        goal_state = int(j) * info.nx + int(i)   # heading 0
        lo = np.array([p.origin[0], p.origin[1], p.origin[2]])
        hi = lo + np.array([p.nx, p.ny, p.nz]) * res
        for name, (radius, t) in tables(lattice, res).items():
            for _ in range(2):   # warm-up: allocation, code objects
                st = ctx.occ_lattice_build(goals, t)
            ts = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                ctx.occ_lattice_build(goals, t)
                ts.append((time.perf_counter() - t0) * 1e3)
            li = ctx.occ_lattice_info()
            batches = -(-li.rounds // ROUNDS_PER_READ)
            row = dict(min_radius=radius, P=int(t.shape[1]), build_ms=spread(ts), rounds=int(li.rounds), tile=int(li.tile), reach=int(li.reach),
                       read_backs_derived=batches, kernel_launches_derived=batches * ROUNDS_PER_READ + 2, stats=[int(v) for v in st], paths={})
            for n in N_STARTS:
                starts = np.zeros(n, capi.LATTICE_POSE_DTYPE)
                starts["xyz"] = rng.uniform(lo, hi, (n, 3)).astype(np.float32)
                starts["h"] = rng.integers(-1, H, n)
                ctx.occ_lattice_paths(starts)
                ts = []
                for _ in range(max(a.reps // 4, 3)):
                    t0 = time.perf_counter()
                    status, _, off, _, _ = ctx.occ_lattice_paths(starts)
                    ts.append((time.perf_counter() - t0) * 1e3)
                row["paths"][str(n)] = dict(ms_median=float(np.median(ts)), ms_min=float(np.min(ts)), routes=int(np.sum(status == 0)), states=int(off[-1]),
                                            longest=int(np.max(np.diff(off.astype(np.int64)))))
            solve_ms, hV = host_solve(cost, t, [goal_state])
            V = ctx.occ_lattice_fetch()
            assert np.array_equal(V, hV), f"{name}: {np.sum(V != hV)} states differ from the host program's"
            row["host"] = dict(fetch_ms=fetch_ms, solve_ms=solve_ms, method="scripts/occ_lattice_host.cpp, g++ -O2, one core", V_agrees=True)
            row["vs_host"] = (fetch_ms + solve_ms) / row["build_ms"]["median"]
            row["vs_plan_build"] = row["build_ms"]["median"] / res_out["plan_build_ms"]["median"]
            res_out["tables"][name] = row
            print(json.dumps({name: row}), file=sys.stderr)
    line = json.dumps(res_out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
