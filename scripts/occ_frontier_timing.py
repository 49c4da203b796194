"""Timing of the frontiers (lv_occ_frontier_build, lv_occ_frontier_rank) over the default 512 x 512 x 64 grid at 0.2 m after the ten
sweeps of scripts/occupancy_timing.py.  Three builds: `planar`, 8-connected over all layers; `planar_above_ground`, the same over a
band of six layers (1.2 m) that starts two layers above the layer holding the most occupied voxels (the ground); and `3d`,
26-connected.  Per build:
  `build_ms_median`, `build_ms_min`  host wall time of lv_occ_frontier_build (the kernels, the two counter read-backs, the stats), over
                  --reps calls after two warm-up calls;
  `stats`         FREE cells, UNKNOWN cells, frontier cells, clusters;
  `kernel_launches_derived`  NOT measured: the build's own kernels (tile, seam, flatten, assign, accumulate, key, number, label, rep),
                  without the passes of the hipcub radix sort, the memsets and the copies;
  `host`          the path the build replaces, timed here: `fetch_ms` (lv_occ_project, or lv_occ_fetch for `3d`), `classify_ms` (the
                  numpy classification of tests/frontier_ref.py: states and frontier mask), `label_ms` (scipy.ndimage.label), and
                  whether its frontier count and its number of components agree with the device's;
  `speedup`       (fetch_ms + classify_ms + label_ms) / build_ms_median.
`rank` (on `planar_above_ground`, after a distance field that counts unknown as an obstacle and a plan whose goal is the observed
cell nearest the grid's centre): median wall time of lv_occ_frontier_rank at reach 0 and 4, and how many clusters have a reached cell.
Everything runs in one child process under a time limit (--timeout seconds).  Prints one JSON line; --out writes it too.

    python scripts/occ_frontier_timing.py --sweeps /tmp/occ_sweeps.npz --out profiles/occ_frontier_timing.json"""
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

OWN_KERNELS = 9
ROBOT_RADIUS, INFLATION_RADIUS = 0.3, 1.0


def timed(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return out, float(np.median(ts)), float(np.min(ts))


def run(a):
    import occupancy_timing

    views, _ = occupancy_timing.make_sweeps(a.sweeps, count_visits=False)
    import lvamd

    lvamd.load()
    from limo_velo_amd import capi, occupancy

    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import frontier_ref as fr
    import occupancy_ref as ocr
    import scipy
    from scipy import ndimage

    res = dict(what="lv_occ_frontier_build / lv_occ_frontier_rank", grid="512x512x64 @ 0.2 m (defaults)", reps=a.reps,
               host_method="numpy + scipy.ndimage.label " + scipy.__version__, cases={})
    with capi.Context() as ctx:
        ctx.occ_configure()
        ctx.occ_integrate(views)
        p = ctx.occ_params()
        prm = ocr.params_of(p)
        per_layer = np.sum(ctx.occ_fetch() >= np.float32(p.l_occ), axis=(1, 2))
        ground = int(np.argmax(per_layer))
        cases = {"planar": dict(planar=1, k_lo=0, k_hi=p.nz - 1, connectivity=8),
                 "planar_above_ground": dict(planar=1, k_lo=ground + 2, k_hi=ground + 7, connectivity=8),
                 "3d": dict(connectivity=26)}
        res["ground_layer"] = ground
        for name, kw in cases.items():
            fp = capi.default_frontier_params(**kw)
            for _ in range(2):   # warm-up: allocation, code objects
                ctx.occ_frontier_build(fp)
            st, med, lo = timed(lambda: ctx.occ_frontier_build(fp), a.reps)
            row = dict(params=kw, build_ms_median=med, build_ms_min=lo, stats=[int(v) for v in st], kernel_launches_derived=OWN_KERNELS)
            planar = bool(kw.get("planar"))
            hreps = 3
            if planar:
                v, fetch_ms, _ = timed(lambda: ctx.occ_project(kw["k_lo"], kw["k_hi"]), hreps)
                classify = lambda: fr.frontier_mask(np.where(v == 100, fr.OCCUPIED, np.where(v == 0, fr.FREE, fr.UNKNOWN)).astype(np.uint8)[None])  # noqa: E731
            else:
                v, fetch_ms, _ = timed(ctx.occ_fetch, hreps)
                classify = lambda: fr.frontier_mask(fr.states(prm, v, fr.fparams()))  # noqa: E731
            mask, classify_ms, _ = timed(classify, hreps)
            (lab, n), label_ms, _ = timed(lambda: fr.components(mask, kw["connectivity"]), hreps)
            row["host"] = dict(fetch_ms=fetch_ms, classify_ms=classify_ms, label_ms=label_ms, frontier_agrees=bool(int(mask.sum()) == int(st[2])),
                               components_agree=bool(n == int(st[3])))
            row["speedup"] = (fetch_ms + classify_ms + label_ms) / med
            res["cases"][name] = row
            print(json.dumps({name: row}), file=sys.stderr)
            del v, mask, lab
        # rank: the band above the ground, unknown = obstacle, the goal at the observed traversable cell nearest the centre
        kw = cases["planar_above_ground"]
        ctx.occ_distance_build(capi.default_distance_params(planar=1, k_lo=kw["k_lo"], k_hi=kw["k_hi"], unknown_is_obstacle=1))
        r = float(p.resolution)
        table = occupancy.inflation_cost_table(r, ROBOT_RADIUS, INFLATION_RADIUS)
        pp = capi.default_plan_params(connectivity=8, min_clear_s2=occupancy.min_clear_s2(r, ROBOT_RADIUS))
        s2, _ = ctx.occ_distance_fetch(metres=False)
        at = np.argwhere((s2 >= int(pp.min_clear_s2)) & (s2 < capi.LV_OCC_FAR))
        j, i = at[np.argmin(((at - np.array(s2.shape) // 2) ** 2).sum(axis=1))]
        goal = np.array([[p.origin[0] + (i + 0.5) * r, p.origin[1] + (j + 0.5) * r, p.origin[2]]], np.float32)
        pst = ctx.occ_plan_build(goal, table, pp)
        st = ctx.occ_frontier_build(capi.default_frontier_params(**kw))
        res["rank"] = dict(goal_cell=[int(i), int(j)], plan_stats=[int(x) for x in pst], clusters=int(st[3]), reach={})
        for reach in (0, 4):
            ctx.occ_frontier_rank(reach)
            (bp, bc), med, lo = timed(lambda: ctx.occ_frontier_rank(reach), a.reps)
            res["rank"]["reach"][str(reach)] = dict(ms_median=med, ms_min=lo, clusters_reached=int(np.sum(bc >= 0)))
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--sweeps", default=None)
    ap.add_argument("--child", action="store_true", help="run in this process")
    ap.add_argument("--timeout", type=int, default=420)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    if a.child:
        return run(a)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps)] + (["--sweeps", a.sweeps] if a.sweeps else [])
    out = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=a.timeout, check=True).stdout.decode().strip().split("\n")
    line = json.dumps(json.loads(out[-1]))
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
