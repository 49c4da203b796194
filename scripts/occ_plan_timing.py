"""Timing of the planner (lv_occ_plan_build, lv_occ_plan_paths) over the default 512 x 512 x 64 grid at 0.2 m after the ten sweeps of
scripts/occupancy_timing.py.  Three cases, one goal each: `planar`, an 8-connected plan over the field of the height band (all
layers: the ground projects as an obstacle); `planar_above_ground`, the same over a band of six layers (1.2 m) that starts two
layers above the layer holding the most occupied voxels (the ground), where routes cross the grid; and `3d`, a 26-connected plan
over the 3-D field.  Per case:
  `build_ms_median`, `build_ms_min`  host wall time of lv_occ_plan_build (cost and seed kernels, the rounds with their read-backs,
                  the stats), over --reps calls after two warm-up calls;
  `rounds`        relaxation rounds of the build, as lv_occ_plan_info reports them (measured);
  `kernel_launches_derived`, `read_backs_derived`  NOT measured: worked out from `rounds` (rounds are launched in batches of
                  PLAN_ROUNDS_PER_READ = 8 between two reads of the round words, plus the cost, seed and stats kernels; the
                  memsets and copies of a build are not counted);
  `stats`         goals used, traversable cells, reached cells, the largest finite P;
  `paths`         for 1, 1024 and 65536 random start points: median wall time of lv_occ_plan_paths (count, scan, fill, copies) and
                  the number of path cells returned.
`host_baseline` (planar fields only): what a caller does without the planner: fetch the distance field (lv_occ_distance_fetch),
build the same graph and run scipy.sparse.csgraph.dijkstra where scipy imports, else the heapq reference of tests/plan_ref.py;
`fetch_ms`, `graph_ms`, `dijkstra_ms` and whether the potential agrees with the device's.  `planar_speedup` is
(fetch_ms + dijkstra_ms) / build_ms_median: the graph assembly in numpy is left out of the host's side.
Each case runs in a child process of its own under a time limit (--case-timeout seconds); the first one that fails ends the run.
Prints one JSON line; --out writes it too.

    python scripts/occ_plan_timing.py --sweeps /tmp/occ_sweeps.npz --out profiles/occ_plan_timing.json"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402

ROUNDS_PER_READ = 8
CASES = {
    "planar": dict(dist=dict(planar=1, k_lo=0, k_hi=63), connectivity=8),
    "planar_above_ground": dict(dist=None, connectivity=8),   # (the band is chosen from the grid: see run_case)
    "3d": dict(dist=dict(), connectivity=26),
}
N_STARTS = (1, 1024, 65536)
ROBOT_RADIUS, INFLATION_RADIUS = 0.3, 1.0


def planar_graph(cost, connectivity=8):
    """(rows, cols, weights) of the planner's graph on a planar cost array [ny, nx], vectorised (the rule of tests/plan_ref.py)."""
    ny, nx = cost.shape
    c = np.zeros((ny + 2, nx + 2), np.int64)
    c[1:-1, 1:-1] = cost
    idx = np.arange(ny * nx).reshape(ny, nx)
    rows, cols, w = [], [], []
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            m = (dx != 0) + (dy != 0)
            if m == 0 or (m == 2 and connectivity == 4):
                continue
            cu = c[1:-1, 1:-1]
            cv = c[1 + dy:ny + 1 + dy, 1 + dx:nx + 1 + dx]
            ok = (cu != 0) & (cv != 0)
            if m == 2:
                ok &= (c[1:-1, 1 + dx:nx + 1 + dx] != 0) & (c[1 + dy:ny + 1 + dy, 1:-1] != 0)
            rows.append(idx[ok])
            cols.append(idx[ok] + dy * nx + dx)
            w.append(((10 if m == 1 else 14) * (cu + cv))[ok])
    return np.concatenate(rows), np.concatenate(cols), np.concatenate(w)


def run_case(a, name):
    import occupancy_timing

    views, _ = occupancy_timing.make_sweeps(a.sweeps, count_visits=False)
    import lvamd

    lvamd.load()
    from limo_velo_amd import capi, occupancy

    case = CASES[name]
    rng = np.random.default_rng(1)
    row = dict(connectivity=case["connectivity"])
    with capi.Context() as ctx:
        ctx.occ_configure()
        ctx.occ_integrate(views)
        p = ctx.occ_params()
        dist = case["dist"]
        if dist is None:
            L = ctx.occ_fetch()
            per_layer = np.sum(L >= np.float32(p.l_occ), axis=(1, 2))
            ground = int(np.argmax(per_layer))
            dist = dict(planar=1, k_lo=ground + 2, k_hi=ground + 7)
            row.update(ground_layer=ground, occupied_in_ground_layer=int(per_layer[ground]))
            del L
        row["distance"] = dist
        ctx.occ_distance_build(capi.default_distance_params(**dist))
        res = float(p.resolution)
        table = occupancy.inflation_cost_table(res, ROBOT_RADIUS, INFLATION_RADIUS)
        pp = capi.default_plan_params(connectivity=case["connectivity"], min_clear_s2=occupancy.min_clear_s2(res, ROBOT_RADIUS))
        # the goal: the centre of the cell nearest the grid's centre that is traversable and sees an obstacle (observed space)
        s2, _ = ctx.occ_distance_fetch(metres=False)
        s3 = s2[None] if s2.ndim == 2 else s2
        at = np.argwhere((s3 >= int(pp.min_clear_s2)) & (s3 < capi.LV_OCC_FAR))
        k, j, i = at[np.argmin(((at - np.array(s3.shape) // 2) ** 2).sum(axis=1))]
        goal = np.array([[p.origin[0] + (i + 0.5) * res, p.origin[1] + (j + 0.5) * res, p.origin[2] + (k + 0.5) * res]], np.float32)
        row["goal_cell"] = [int(i), int(j), int(k)]
        for _ in range(2):   # warm-up: allocation, code objects
            st = ctx.occ_plan_build(goal, table, pp)
        ts = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            ctx.occ_plan_build(goal, table, pp)
            ts.append((time.perf_counter() - t0) * 1e3)
        info = ctx.occ_plan_info()
        batches = -(-info.rounds // ROUNDS_PER_READ)
        row.update(build_ms_median=float(np.median(ts)), build_ms_min=float(np.min(ts)), build_ms_max=float(np.max(ts)), rounds=int(info.rounds),
                   read_backs_derived=batches, kernel_launches_derived=batches * ROUNDS_PER_READ + 3, stats=[int(v) for v in st],
                   table=[int(v) for v in table], min_clear_s2=int(pp.min_clear_s2), field=[info.nx, info.ny, info.nz], paths={})
        lo = np.array([p.origin[0], p.origin[1], p.origin[2]])
        hi = lo + np.array([p.nx, p.ny, p.nz]) * res
        for n in N_STARTS:
            starts = rng.uniform(lo, hi, (n, 3)).astype(np.float32)
            ctx.occ_plan_paths(starts)
            ts = []
            for _ in range(max(a.reps // 4, 3)):
                t0 = time.perf_counter()
                status, cost, off, cells = ctx.occ_plan_paths(starts)
                ts.append((time.perf_counter() - t0) * 1e3)
            row["paths"][str(n)] = dict(ms_median=float(np.median(ts)), ms_min=float(np.min(ts)), routes=int(np.sum(status == 0)),
                                        cells=int(off[-1]), longest=int(np.max(np.diff(off.astype(np.int64)))))
        if name.startswith("planar") and not a.no_host:
            P, cc = ctx.occ_plan_fetch()
            ts = []
            for _ in range(3):
                t0 = time.perf_counter()
                s2, _ = ctx.occ_distance_fetch(metres=False)
                ts.append((time.perf_counter() - t0) * 1e3)
            host = dict(fetch_ms=float(np.median(ts)))
            sys.path.insert(0, os.path.join(ROOT, "tests"))
            import plan_ref as pr

            hc = pr.cell_cost(s2, int(pp.min_clear_s2), table)
            host["cost_agrees"] = bool(np.array_equal(hc, cc))
            goals_at = np.nonzero(P.reshape(-1) == 0)[0]
            t0 = time.perf_counter()
            r, c, w = planar_graph(hc, case["connectivity"])
            host["graph_ms"] = (time.perf_counter() - t0) * 1e3
            try:
                import scipy
                from scipy.sparse import csr_matrix
                from scipy.sparse.csgraph import dijkstra

                g = csr_matrix((w.astype(np.float64), (r, c)), shape=(hc.size, hc.size))
                t0 = time.perf_counter()
                d = dijkstra(g, directed=True, indices=goals_at, min_only=True)
                host.update(dijkstra_ms=(time.perf_counter() - t0) * 1e3, method="scipy.sparse.csgraph.dijkstra " + scipy.__version__)
                hP = np.where(np.isfinite(d), d, pr.UNREACHED).astype(np.uint32)
            except ImportError:
                adj = {}
                for u, v, e in zip(r.tolist(), c.tolist(), w.tolist()):
                    adj.setdefault(u, []).append((v, e))
                t0 = time.perf_counter()
                hP = pr.dijkstra(hc.size, adj, goals_at.tolist())
                host.update(dijkstra_ms=(time.perf_counter() - t0) * 1e3, method="heapq (tests/plan_ref.py)")
            host["potential_agrees"] = bool(np.array_equal(hP, P.reshape(-1)))
            row["host_baseline"] = host
            row["planar_speedup"] = (host["fetch_ms"] + host["dijkstra_ms"]) / row["build_ms_median"]
    print(json.dumps(row))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--sweeps", default=None)
    ap.add_argument("--case", default=None, choices=sorted(CASES), help="this case only, in this process")
    ap.add_argument("--case-timeout", type=int, default=240)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-host", action="store_true")
    a = ap.parse_args()
    if a.case:
        return run_case(a, a.case)
    res = dict(what="lv_occ_plan_build / lv_occ_plan_paths", grid="512x512x64 @ 0.2 m (defaults)", reps=a.reps, rounds_per_read=ROUNDS_PER_READ,
               cases={})
    for name in CASES:   # a fresh child per case, each under its own time limit; nothing more is started after a failure
        cmd = [sys.executable, os.path.abspath(__file__), "--case", name, "--reps", str(a.reps)] + (["--sweeps", a.sweeps] if a.sweeps else []) + \
              (["--no-host"] if a.no_host else [])
        out = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=a.case_timeout, check=True).stdout.decode().strip().split("\n")
        res["cases"][name] = json.loads(out[-1])
        print(json.dumps({name: res["cases"][name]}), file=sys.stderr)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
